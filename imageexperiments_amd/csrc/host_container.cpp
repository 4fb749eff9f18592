// host_container.cpp -- product host code: the ".mn" container (see host_bitstream.h): header, the per-stream wrapper, the routes
// from streams, records and device-assembled symbols to a container, and the parser.  Everything per symbol or per bit is
// host_bitstream.cpp's; this file calls it once per stream.
#include "host_bitstream.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace mpc {

namespace {
constexpr uint32_t kMagic = 0x4D4E3234u;        // CompressedImage.cpp:14

size_t tile_count(int width, int height, int block_size) {
    return static_cast<size_t>((width + block_size - 1) / block_size) * static_cast<size_t>((height + block_size - 1) / block_size);
}

// writeCompressed's header (:410-427): the quantiser steps as u16, quant[ch * channel_stride + i]
void write_header(BitWriter& out, int width, int height, int K, int block_size, const uint16_t* quant, size_t channel_stride) {
    out.put(kMagic, 32);
    out.put(static_cast<uint32_t>(width), 32);
    out.put(static_cast<uint32_t>(height), 32);
    out.put(static_cast<uint8_t>(K), 8);
    out.put(static_cast<uint8_t>(block_size), 8);
    for (int ch = 0; ch < 3; ++ch)
        for (int i = 0; i < K; ++i) out.put(quant[static_cast<size_t>(ch) * channel_stride + static_cast<size_t>(i)], 16);
}

// readCompressed's (:640-655), with its checks; `in` is left in front of the quantiser steps
bool read_header(BitReader& in, int* width, int* height, int* K, int* block_size) {
    if (static_cast<uint32_t>(in.get(32)) != kMagic) return false;
    *width = static_cast<int>(in.get(32));
    *height = static_cast<int>(in.get(32));
    *K = static_cast<int>(in.get(8));
    *block_size = static_cast<int>(in.get(8));
    return !(*K < 1 || *K > 32 || *block_size < 1 || *block_size > 8 || *width < 1 || *height < 1);
}

// writeCompressed's size rule (:450): a stream is run-length coded where that saves more than four symbols
bool rle_pays(size_t packed_size, size_t n) { return packed_size + 4 < n; }

// One stream of codes as the container holds it (:449-453): run-length flag, the packed size where set, Huffman or Golomb
void code_stream(const uint16_t* data, size_t n, BitWriter& w) {
    const bool shorter = rle_pays(rle_encoded_size(data, n), n);
    w.put(shorter ? 1 : 0, 1);
    if (!shorter) {
        write_huffman_or_golomb(data, n, w);
        return;
    }
    const std::vector<uint16_t> packed = rle_encode(data, n);
    w.put(static_cast<uint32_t>(packed.size()), 32);
    write_huffman_or_golomb(packed.data(), packed.size(), w);
}

std::vector<uint16_t> dc_difference(const std::vector<uint16_t>& v) {       // :428-446
    std::vector<uint16_t> out(v.size());
    int32_t prev = 0;
    for (size_t i = 0; i < v.size(); ++i) {
        out[i] = static_cast<uint16_t>(zigzag_encode(static_cast<int32_t>(v[i]) - prev));
        prev = static_cast<int32_t>(v[i]);
    }
    return out;
}
}  // namespace

BitWriter container_head(int width, int height, int K, int block_size, const double* quant) {
    std::vector<uint16_t> carried(3 * static_cast<size_t>(K));
    for (size_t i = 0; i < carried.size(); ++i) carried[i] = header_quant(quant[i]);      // :420 u16 of an integral double
    BitWriter head;
    write_header(head, width, height, K, block_size, carried.data(), static_cast<size_t>(K));
    return head;
}

std::vector<uint8_t> write_compressed(const Streams& s) {
    const int K = s.K;
    BitWriter out;
    write_header(out, s.width, s.height, K, s.block_size, &s.quant[0][0], sizeof(s.quant[0]) / sizeof(s.quant[0][0]));
    std::vector<BitWriter> parts(static_cast<size_t>(6 * K + 1));
    parallel_jobs(6 * K + 1, [&](int job) {
        BitWriter& w = parts[static_cast<size_t>(job)];
        if (job == 0) {
            write_huffman_or_golomb(s.lengths.data(), s.lengths.size(), w);
            return;
        }
        const int i = job - 1;
        const bool dc = (i == 1 || i == 2 * K + 1 || i == 4 * K + 1);
        const std::vector<uint16_t> diffed = dc ? dc_difference(s.codes[i]) : std::vector<uint16_t>();
        const std::vector<uint16_t>& stream = dc ? diffed : s.codes[i];
        code_stream(stream.data(), stream.size(), w);
    });
    for (const BitWriter& w : parts) out.append(w);
    return out.bytes();
}

// Records to the container's 1 + 6K parts without materialising the 6K streams of a frame (hundreds of MB of freshly faulted
// pages at K = 32): one job per (channel, step) gathers its two streams into buffers the worker thread keeps between calls and
// codes them straight into its part of the container.  Same bytes as streams built first and given to write_compressed.
namespace {
// record (tile t, channel ch, step i) = choices[t * tile_stride + ch * channel_stride + i * step_stride]
struct RecordLayout {
    size_t tile_stride, channel_stride, step_stride;
};

std::vector<BitWriter> code_records(int width, int height, int K, int block_size, const uint16_t* counts, const uint32_t* choices,
                                    const RecordLayout& layout) {
    const size_t tiles = tile_count(width, height, block_size);
    std::vector<BitWriter> parts(static_cast<size_t>(6 * K + 1));
    // the big jobs first: step 0 of every channel holds every tile-channel, later steps fewer
    parallel_jobs(3 * K + 1, [&](int job0) {
        if (job0 == 0) {
            write_huffman_or_golomb(counts, 3 * tiles, parts[0]);                              // the lengths stream: the longest
            return;
        }
        const int job = job0 - 1;
        const int i = job / 3, ch = job - 3 * i;                 // job order: (step 0: Y U V), (step 1: Y U V), ...
        thread_local std::vector<uint16_t> d, c;
        const uint32_t* mine = choices + static_cast<size_t>(ch) * layout.channel_stride + static_cast<size_t>(i) * layout.step_stride;
        const size_t tile_stride = layout.tile_stride;
        d.clear();
        c.clear();
        for (size_t t = 0; t < tiles; ++t) {
            if (counts[3 * t + static_cast<size_t>(ch)] > i) {
                const uint32_t rec = mine[t * tile_stride];
                d.push_back(static_cast<uint16_t>(rec & 0xFFFFu));
                c.push_back(static_cast<uint16_t>(rec >> 16));
            }
        }
        const int index = 2 * K * ch + 2 * i;                    // codes[index] = deltaId, [index + 1] = intCoeff
        code_stream(d.data(), d.size(), parts[static_cast<size_t>(index + 1)]);
        if (i == 0) c = dc_difference(c);                        // DC: the step-0 coefficients (:428-446)
        code_stream(c.data(), c.size(), parts[static_cast<size_t>(index + 2)]);
    });
    return parts;
}

// Concatenate head and parts bit-wise into big-endian bytes in a malloc'ed buffer.  Every part knows its bit offset, so
// the parts are shifted into place in parallel; only the two words a part may share with its neighbours are merged
// with atomic ORs (into words cleared beforehand), everything in between is a plain store.
uint8_t* concat_malloc(const BitWriter& head, const std::vector<BitWriter>& parts, size_t* nbytes) {
    std::vector<size_t> offset(parts.size() + 1);
    size_t total = head.bit_size();
    for (size_t p = 0; p < parts.size(); ++p) {
        offset[p] = total;
        total += parts[p].bit_size();
    }
    offset[parts.size()] = total;
    const size_t nwords = (total + 63) / 64;
    uint64_t* dst = static_cast<uint64_t*>(std::malloc((nwords ? nwords : 1) * sizeof(uint64_t)));
    if (!dst) return nullptr;
    auto place = [dst](const BitWriter& w, size_t bit_offset) {
        const size_t nbits = w.bit_size();
        if (nbits == 0) return;
        const uint64_t* src = w.words();
        const size_t src_words = (nbits + 63) / 64;
        const size_t w0 = bit_offset >> 6, last = (bit_offset + nbits - 1) >> 6;
        const int shift = static_cast<int>(bit_offset & 63);
        for (size_t d = w0; d <= last; ++d) {                   // destination word d = source bits [64(d-w0) - shift, +64)
            const size_t i = d - w0;
            uint64_t v = 0;
            if (shift == 0) v = i < src_words ? src[i] : 0;
            else {
                if (i < src_words) v |= src[i] >> shift;
                if (i >= 1 && i - 1 < src_words) v |= src[i - 1] << (64 - shift);
            }
            const uint64_t be = __builtin_bswap64(v);            // MSB-first bit order = big-endian bytes
            if (d == w0 || d == last) __atomic_fetch_or(&dst[d], be, __ATOMIC_RELAXED);
            else dst[d] = be;
        }
    };
    // clear the words that can be shared between neighbours (first and last word of every piece)
    auto clear_ends = [dst](size_t bit_offset, size_t nbits) {
        if (nbits == 0) return;
        dst[bit_offset >> 6] = 0;
        dst[(bit_offset + nbits - 1) >> 6] = 0;
    };
    clear_ends(0, head.bit_size());
    for (size_t p = 0; p < parts.size(); ++p) clear_ends(offset[p], parts[p].bit_size());
    place(head, 0);
    parallel_jobs(static_cast<int>(parts.size()), [&](int p) { place(parts[static_cast<size_t>(p)], offset[static_cast<size_t>(p)]); });
    *nbytes = (total + 7) / 8;
    return reinterpret_cast<uint8_t*>(dst);
}
}  // namespace

// records in the reference's visiting order, choices[(t * 3 + ch) * K + i]
uint8_t* encode_records_malloc(int width, int height, int K, int block_size, const double* quant, const uint16_t* counts,
                               const uint32_t* choices, size_t* nbytes) {
    const RecordLayout layout{3 * static_cast<size_t>(K), static_cast<size_t>(K), 1};
    return concat_malloc(container_head(width, height, K, block_size, quant), code_records(width, height, K, block_size, counts, choices, layout), nbytes);
}

uint8_t* encode_planar_records_malloc(int width, int height, int K, int block_size, const double* quant, const uint16_t* counts,
                                      const uint32_t* planar, size_t* nbytes) {
    const size_t tiles = tile_count(width, height, block_size);
    const RecordLayout layout{1, static_cast<size_t>(K) * tiles, tiles};
    return concat_malloc(container_head(width, height, K, block_size, quant), code_records(width, height, K, block_size, counts, planar, layout), nbytes);
}

// The container from streams the device has already assembled (mp_streams.hip): `symbols` holds codes[0], codes[1], ... codes[6K-1]
// back to back (stream s = symbols[off[s] .. off[s+1])), live symbols only, in the reference's tile order, the three step-0
// coefficient streams already difference coded.  One job per stream (the lengths stream first: the longest).
uint8_t* encode_symbol_streams_malloc(int width, int height, int K, int block_size, const double* quant, const uint16_t* counts,
                                      const uint16_t* symbols, const unsigned long long* off, size_t* nbytes) {
    const size_t tiles = tile_count(width, height, block_size);
    std::vector<BitWriter> parts(static_cast<size_t>(6 * K + 1));
    // longest jobs first: the lengths stream, then the streams in the order of their sizes
    std::vector<int> order(static_cast<size_t>(6 * K));
    for (int s = 0; s < 6 * K; ++s) order[static_cast<size_t>(s)] = s;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return off[x + 1] - off[x] > off[y + 1] - off[y]; });
    parallel_jobs(6 * K + 1, [&](int job) {
        if (job == 0) {
            write_huffman_or_golomb(counts, 3 * tiles, parts[0]);
            return;
        }
        const int s = order[static_cast<size_t>(job - 1)];
        code_stream(symbols + off[s], static_cast<size_t>(off[s + 1] - off[s]), parts[static_cast<size_t>(s + 1)]);
    });
    return concat_malloc(container_head(width, height, K, block_size, quant), parts, nbytes);
}

// encode_symbol_streams_malloc by the route the device-side entropy stage takes, with the device's share done here on the
// host: per-stream statistics -> plan_stream -> codes at the planned bit offsets -> OR the pieces into place.  Exists so that
// the planning half can be checked against the direct route without a GPU (tests/test_host_bitstream.py).
uint8_t* encode_symbol_streams_by_plan_malloc(int width, int height, int K, int block_size, const double* quant, const uint16_t* counts,
                                              const uint16_t* symbols, const unsigned long long* off, size_t* nbytes) {
    const size_t tiles = tile_count(width, height, block_size);
    const int S = 6 * K + 1;
    std::vector<StreamPlan> plans(static_cast<size_t>(S));
    std::vector<BitWriter> payload(static_cast<size_t>(S));
    for (int j = 0; j < S; ++j) {
        const uint16_t* data = j == 0 ? counts : symbols + off[j - 1];
        const size_t n = j == 0 ? 3 * tiles : static_cast<size_t>(off[j] - off[j - 1]);
        const size_t rle_size = j == 0 ? n : rle_encoded_size(data, n);
        const bool shorter = j != 0 && rle_pays(rle_size, n);
        const std::vector<uint16_t> packed = shorter ? rle_encode(data, n) : std::vector<uint16_t>();
        const uint16_t* coded = shorter ? packed.data() : data;
        const size_t coded_n = shorter ? packed.size() : n;
        std::vector<uint32_t> hist(65536, 0), first(65536, 0), triples;
        uint32_t largest = 0;
        for (size_t i = 0; i < coded_n; ++i) {
            if (hist[coded[i]]++ == 0) first[coded[i]] = static_cast<uint32_t>(i);
            largest = std::max<uint32_t>(largest, coded[i]);
        }
        for (uint32_t v = 0; v < 65536; ++v)
            if (hist[v]) { triples.push_back(v); triples.push_back(hist[v]); triples.push_back(first[v]); }
        StreamPlan& p = plans[static_cast<size_t>(j)];
        plan_stream(j != 0, shorter, static_cast<uint32_t>(rle_size), coded_n, largest, triples.data(), triples.size() / 3, p);
        BitWriter& w = payload[static_cast<size_t>(j)];
        if (p.mode == 0) {
            std::vector<uint32_t> code_of(static_cast<size_t>(largest) + 1, 0);
            std::vector<uint8_t> length_of(static_cast<size_t>(largest) + 1, 0);
            for (size_t k = 0; k < p.entries.size(); k += 3) {
                code_of[p.entries[k]] = p.entries[k + 1];
                length_of[p.entries[k]] = static_cast<uint8_t>(p.entries[k + 2]);
            }
            w.put_codes(coded, coded_n, code_of.data(), length_of.data(), p.payload_bits);
        } else {
            golomb_encode(coded, coded_n, p.m, w);
        }
        if (w.bit_size() != p.payload_bits) return nullptr;
    }
    const BitWriter head = container_head(width, height, K, block_size, quant);
    size_t total = head.bit_size();
    for (int j = 0; j < S; ++j) total += plans[static_cast<size_t>(j)].pre.bit_size() + plans[static_cast<size_t>(j)].payload_bits + plans[static_cast<size_t>(j)].post.bit_size();
    *nbytes = (total + 7) / 8;
    uint8_t* dst = static_cast<uint8_t*>(std::calloc(*nbytes ? *nbytes : 1, 1));
    if (!dst) return nullptr;
    or_bits(dst, *nbytes, 0, head);
    size_t at = head.bit_size();
    for (int j = 0; j < S; ++j) {
        const StreamPlan& p = plans[static_cast<size_t>(j)];
        or_bits(dst, *nbytes, at, p.pre);
        at += p.pre.bit_size();
        or_bits(dst, *nbytes, at, payload[static_cast<size_t>(j)]);
        at += p.payload_bits;
        or_bits(dst, *nbytes, at, p.post);
        at += p.post.bit_size();
    }
    return dst;
}

// The serial half of readCompressed: everything the format chains from one code to the next (the codes are self-delimiting and
// a stream's table sits where the stream before it ended), and nothing else.  No worker pool, no shared state: safe on several
// threads at once.
bool read_compressed_coded(const uint8_t* bytes, size_t nbytes, CodedStreams& s) {
    BitReader in(bytes, nbytes);
    if (!read_header(in, &s.width, &s.height, &s.K, &s.block_size)) return false;
    const int K = s.K;
    for (int ch = 0; ch < 3; ++ch)
        for (int i = 0; i < K; ++i) s.quant[ch][i] = static_cast<uint16_t>(in.get(16));
    const size_t tiles = tile_count(s.width, s.height, s.block_size);
    s.lengths.clear();
    if (tiles > (static_cast<size_t>(1) << 40) / 3) return false;
    if (!read_huffman_or_golomb(in, 3 * tiles, s.lengths)) return false;
    // a Huffman-coded lengths stream carries its own end: it must still describe exactly this frame's tiles (the
    // device decoder walks tiles_x * tiles_y records)
    if (s.lengths.size() != 3 * tiles) return false;
    s.codes.assign(static_cast<size_t>(6 * K), {});
    // length of an un-packed stream = tile-channels of its layer with more than `depth` atoms (:680-685): suffix sums
    // of the histogram of lengths, once for all 6K streams
    std::vector<size_t> expect_of(static_cast<size_t>(3 * K), 0);
    {
        std::vector<size_t> hist(static_cast<size_t>(3) * 65536, 0);
        for (size_t t = 0; t < s.lengths.size() / 3; ++t)
            for (size_t layer = 0; layer < 3; ++layer) ++hist[layer * 65536 + s.lengths[3 * t + layer]];
        for (size_t layer = 0; layer < 3; ++layer) {
            size_t above = 0;
            for (int v = 65535; v > K; --v) above += hist[layer * 65536 + static_cast<size_t>(v)];
            for (int depth = K - 1; depth >= 0; --depth) {
                above += hist[layer * 65536 + static_cast<size_t>(depth + 1)];
                expect_of[layer * static_cast<size_t>(K) + static_cast<size_t>(depth)] = above;
            }
        }
    }
    // Only the entropy codes are undone here: run-length expansion (:660-678) and the DC sums (:690-705) of a stream need nothing
    // from the streams behind it (read_compressed does them on the pool, the sequence decoder on the device).
    s.packed.assign(static_cast<size_t>(6 * K), 0);
    s.expect.assign(static_cast<size_t>(6 * K), 0);
    for (int i = 0; i < 6 * K; ++i) {
        s.expect[i] = expect_of[(static_cast<size_t>(i / 2) / K) * static_cast<size_t>(K) + static_cast<size_t>(i / 2) % K];
        if (in.get(1) == 1) {
            const size_t packed_len = static_cast<size_t>(in.get(32));
            s.packed[i] = 1;
            if (!read_huffman_or_golomb(in, packed_len, s.codes[i])) return false;
            // At most every third symbol of a run-length coded stream is a count and every other symbol expands to itself: a
            // stream of n symbols expands to at least n - n/3.  More than the lengths stream allows cannot be valid, and whoever
            // expands the stream may size its buffers by `expect`.
            if (s.codes[i].size() - s.codes[i].size() / 3 > s.expect[i]) return false;
        } else {
            if (!read_huffman_or_golomb(in, s.expect[i], s.codes[i])) return false;
        }
    }
    return true;
}

bool read_compressed(const uint8_t* bytes, size_t nbytes, Streams& s) {
    CodedStreams c;
    if (!read_compressed_coded(bytes, nbytes, c)) return false;
    const std::vector<uint8_t> is_packed = std::move(c.packed);
    const std::vector<size_t> expect = std::move(c.expect);
    s = std::move(static_cast<Streams&>(c));
    const int K = s.K;
    std::vector<char> bad(static_cast<size_t>(6 * K), 0);
    parallel_jobs(6 * K, [&](int i) {
        if (is_packed[i]) {
            // run lengths come from the data: refuse to expand beyond what the lengths stream allows for this stream
            const std::vector<uint16_t> packed = std::move(s.codes[i]);
            size_t expanded = 0;
            if (!rle_decoded_size(packed.data(), packed.size(), expect[i], &expanded)) { bad[i] = 1; return; }
            s.codes[i] = rle_decode(packed.data(), packed.size());
        }
        if (s.codes[i].size() != expect[i]) { bad[i] = 1; return; }
        if (i == 1 || i == 2 * K + 1 || i == 4 * K + 1) {       // :690-705
            int32_t acc = 0;
            for (uint16_t& c : s.codes[i]) {
                acc += zigzag_decode(c);
                c = static_cast<uint16_t>(acc);
            }
        }
    });
    for (int i = 0; i < 6 * K; ++i)
        if (bad[i]) return false;
    return true;
}

// the header alone (CompressedImage.cpp:640-655), with read_compressed's checks of it
bool container_info(const uint8_t* bytes, size_t nbytes, int* width, int* height, int* K, int* block_size) {
    if (nbytes < 14) return false;
    BitReader in(bytes, nbytes);
    return read_header(in, width, height, K, block_size);
}

bool disassemble_streams(const Streams& s, uint16_t* counts, uint32_t* choices) {
    const int K = s.K;
    const size_t n = s.lengths.size(), tiles = n / 3;
    if (n % 3 != 0) return false;
    for (int i = 0; i < 6 * K; i += 2)
        if (s.codes[i].size() != s.codes[i + 1].size()) return false;
    // Blocks of tiles in parallel: where a block starts in each of the 3K stream pairs = tile-channels of the blocks in front of
    // it with more than `step` atoms (suffix sums of a histogram of the block's counts, then a running sum over the blocks).
    const size_t block = 4096, blocks = (tiles + block - 1) / block;
    std::vector<size_t> start((blocks + 1) * static_cast<size_t>(3 * K), 0);
    std::vector<char> bad(blocks, 0);
    parallel_jobs(static_cast<int>(blocks), [&](int b) {
        std::vector<size_t> hist(static_cast<size_t>(3 * (K + 1)), 0);
        const size_t lo = block * static_cast<size_t>(b), hi = std::min(tiles, lo + block);
        for (size_t o = 3 * lo; o < 3 * hi; ++o) {
            if (s.lengths[o] > K) { bad[b] = 1; return; }
            ++hist[(o % 3) * static_cast<size_t>(K + 1) + s.lengths[o]];
        }
        size_t* mine = start.data() + (static_cast<size_t>(b) + 1) * static_cast<size_t>(3 * K);
        for (int ch = 0; ch < 3; ++ch) {
            size_t above = 0;
            for (int i = K - 1; i >= 0; --i) {
                above += hist[static_cast<size_t>(ch) * (K + 1) + static_cast<size_t>(i + 1)];
                mine[ch * K + i] = above;
            }
        }
    });
    for (size_t b = 0; b < blocks; ++b)
        if (bad[b]) return false;
    for (size_t b = 1; b <= blocks; ++b)
        for (int p = 0; p < 3 * K; ++p) start[b * static_cast<size_t>(3 * K) + p] += start[(b - 1) * static_cast<size_t>(3 * K) + p];
    for (int p = 0; p < 3 * K; ++p)                                 // every stream must hold what the lengths promise
        if (start[blocks * static_cast<size_t>(3 * K) + p] > s.codes[2 * p].size()) return false;
    parallel_jobs(static_cast<int>(blocks), [&](int b) {
        std::vector<size_t> cursor(start.begin() + static_cast<size_t>(b) * (3 * K), start.begin() + (static_cast<size_t>(b) + 1) * (3 * K));
        const size_t lo = block * static_cast<size_t>(b), hi = std::min(tiles, lo + block);
        for (size_t o = 3 * lo; o < 3 * hi; ++o) {
            const int ch = static_cast<int>(o % 3);
            const int count = s.lengths[o];
            counts[o] = s.lengths[o];
            for (int i = 0; i < count; ++i) {
                const size_t at = cursor[static_cast<size_t>(ch * K + i)]++;
                choices[o * K + i] = static_cast<uint32_t>(s.codes[2 * K * ch + 2 * i][at]) | (static_cast<uint32_t>(s.codes[2 * K * ch + 2 * i + 1][at]) << 16);
            }
        }
    });
    return true;
}

bool disassemble_streams(const Streams& s, std::vector<uint16_t>& counts, std::vector<uint32_t>& choices) {
    counts.assign(s.lengths.size(), 0);
    choices.assign(s.lengths.size() * static_cast<size_t>(s.K), 0);
    return disassemble_streams(s, counts.data(), choices.data());
}

}  // namespace mpc
