// host_container.cpp -- product host code: the ".mn" container (see host_bitstream.h): header, the per-stream wrapper, the routes
// from streams, records and device-assembled symbols to a container, and the parser.  Everything per symbol or per bit is
// host_bitstream.cpp's; this file calls it once per stream.
#include "host_bitstream.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
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
namespace {
void index_aux_pass(const uint16_t* v, size_t n, uint32_t interval, bool packed, bool dc, std::vector<IndexAux>& aux);

// interval 0: the container alone.  Otherwise cps gets, stream behind stream, the container bit of every interval-th coded
// symbol, and `planned` where each stream's codes begin; *wide: a Huffman code longer than 32 bits, nothing recorded.  auxs
// (optional, with an interval): index version 2's aux entries of the streams that have any, stream behind stream, two words each
// as the blob holds them -- index_aux_pass over the coded symbols, which is what the device's pack pass and sums must equal
uint8_t* encode_by_plan(int width, int height, int K, int block_size, const double* quant, const uint16_t* counts, const uint16_t* symbols,
                        const unsigned long long* off, uint32_t interval, size_t* nbytes, std::vector<StreamPlan>& plans,
                        std::vector<PlannedStream>& planned, std::vector<uint64_t>& cps, bool* wide,
                        std::vector<uint64_t>* auxs = nullptr) {
    const size_t tiles = tile_count(width, height, block_size);
    const int S = 6 * K + 1;
    plans.assign(static_cast<size_t>(S), StreamPlan());
    planned.assign(static_cast<size_t>(S), PlannedStream());
    cps.clear();
    if (auxs) auxs->clear();
    *wide = false;
    std::vector<BitWriter> payload(static_cast<size_t>(S));
    size_t bit = container_head(width, height, K, block_size, quant).bit_size();
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
        PlannedStream& ps = planned[static_cast<size_t>(j)];
        bit += p.pre.bit_size();
        ps.first_code_bit = bit;
        ps.n = n;
        ps.eff_n = coded_n;
        ps.shorter = shorter;
        if (p.mode == 0 && p.max_code_length > 32) *wide = true;
        const bool record = interval != 0 && !*wide;
        if (record && auxs && index_stream_has_aux(static_cast<size_t>(j), K, shorter)) {
            std::vector<IndexAux> entries;
            index_aux_pass(coded, coded_n, interval, shorter, (j - 1) % (2 * K) == 1, entries);
            for (const IndexAux& e : entries) {
                auxs->push_back(e.out);
                auxs->push_back(static_cast<uint64_t>(e.prev) | (static_cast<uint64_t>(e.dc) << 16) | (static_cast<uint64_t>(e.state) << 32));
            }
        }
        BitWriter& w = payload[static_cast<size_t>(j)];
        if (p.mode == 0) {
            std::vector<uint32_t> code_of(static_cast<size_t>(largest) + 1, 0);
            std::vector<uint8_t> length_of(static_cast<size_t>(largest) + 1, 0);
            for (size_t k = 0; k < p.entries.size(); k += 3) {
                code_of[p.entries[k]] = p.entries[k + 1];
                length_of[p.entries[k]] = static_cast<uint8_t>(p.entries[k + 2]);
            }
            if (!record) w.put_codes(coded, coded_n, code_of.data(), length_of.data(), p.payload_bits);
            else
                for (size_t i = 0; i < coded_n; ++i) {           // the device's walk: the position in front of every code
                    if (i % interval == 0) cps.push_back(bit + w.bit_size());
                    w.put(code_of[coded[i]], length_of[coded[i]]);
                }
        } else if (!record) {
            golomb_encode(coded, coded_n, p.m, w);
        } else {
            for (size_t i = 0; i < coded_n; ++i) {
                if (i % interval == 0) cps.push_back(bit + w.bit_size());
                golomb_write(coded[i], p.m, w);
            }
        }
        if (w.bit_size() != p.payload_bits) return nullptr;
        bit += p.payload_bits + p.post.bit_size();
    }
    const BitWriter head = container_head(width, height, K, block_size, quant);
    *nbytes = (bit + 7) / 8;
    uint8_t* dst = static_cast<uint8_t*>(std::calloc(*nbytes ? *nbytes : 1, 1));
    if (!dst) return nullptr;
    or_bits(dst, *nbytes, 0, head);
    for (int j = 0; j < S; ++j) {
        const StreamPlan& p = plans[static_cast<size_t>(j)];
        const size_t at = static_cast<size_t>(planned[static_cast<size_t>(j)].first_code_bit);
        or_bits(dst, *nbytes, at - p.pre.bit_size(), p.pre);
        or_bits(dst, *nbytes, at, payload[static_cast<size_t>(j)]);
        or_bits(dst, *nbytes, at + p.payload_bits, p.post);
    }
    return dst;
}
}  // namespace

uint8_t* encode_symbol_streams_by_plan_malloc(int width, int height, int K, int block_size, const double* quant, const uint16_t* counts,
                                              const uint16_t* symbols, const unsigned long long* off, size_t* nbytes) {
    std::vector<StreamPlan> plans;
    std::vector<PlannedStream> planned;
    std::vector<uint64_t> cps;
    bool wide;
    return encode_by_plan(width, height, K, block_size, quant, counts, symbols, off, 0, nbytes, plans, planned, cps, &wide);
}

uint8_t* encode_symbol_streams_by_plan_indexed_malloc(int width, int height, int K, int block_size, const double* quant,
                                                      const uint16_t* counts, const uint16_t* symbols, const unsigned long long* off,
                                                      uint32_t interval, size_t* nbytes, std::vector<uint8_t>& index, bool expanded) {
    index.clear();
    const bool consistent = streams_match_lengths(counts, tile_count(width, height, block_size), K, off);
    std::vector<StreamPlan> plans;
    std::vector<PlannedStream> planned;
    std::vector<uint64_t> cps, auxs;
    bool wide = false;
    uint8_t* dst = encode_by_plan(width, height, K, block_size, quant, counts, symbols, off, consistent ? interval : 0, nbytes, plans,
                                  planned, cps, &wide, expanded ? &auxs : nullptr);
    if (!dst || !consistent) return dst;
    const size_t head_bits = container_head(width, height, K, block_size, quant).bit_size();
    const bool ok = wide ? build_container_index(dst, *nbytes, interval, index, expanded)
                         : index_from_plan(interval, *nbytes, width, height, K, block_size, head_bits, plans.data(), planned.data(),
                                           6 * K + 1, cps.data(), index, expanded, auxs.data(), auxs.size() / 2);
    if (!ok) {
        std::free(dst);
        return nullptr;
    }
    return dst;
}

// The serial half of readCompressed: everything the format chains from one code to the next (the codes are self-delimiting and
// a stream's table sits where the stream before it ended), and nothing else.  No worker pool, no shared state: safe on several
// threads at once.
namespace {
// read_compressed_coded; bounds (optional): [1 + 6K + 1] the bit each stream's wrapper begins at, and the bit behind the last stream
bool parse_coded(const uint8_t* bytes, size_t nbytes, CodedStreams& s, std::vector<size_t>* bounds) {
    BitReader in(bytes, nbytes);
    if (!read_header(in, &s.width, &s.height, &s.K, &s.block_size)) return false;
    const int K = s.K;
    for (int ch = 0; ch < 3; ++ch)
        for (int i = 0; i < K; ++i) s.quant[ch][i] = static_cast<uint16_t>(in.get(16));
    const size_t tiles = tile_count(s.width, s.height, s.block_size);
    s.lengths.clear();
    if (tiles > (static_cast<size_t>(1) << 40) / 3) return false;
    if (bounds) bounds->assign(1, in.position());
    if (!read_huffman_or_golomb(in, 3 * tiles, s.lengths)) return false;
    // a Huffman-coded lengths stream carries its own end: it must still describe exactly this frame's tiles (the
    // device decoder walks tiles_x * tiles_y records)
    if (s.lengths.size() != 3 * tiles) return false;
    s.codes.assign(static_cast<size_t>(6 * K), {});
    // Only the entropy codes are undone here: run-length expansion (:660-678) and the DC sums (:690-705) of a stream need nothing
    // from the streams behind it (read_compressed does them on the pool, the sequence decoder on the device).
    s.packed.assign(static_cast<size_t>(6 * K), 0);
    s.expect = expected_sizes(s.lengths, K);
    for (int i = 0; i < 6 * K; ++i) {
        if (bounds) bounds->push_back(in.position());
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
    if (bounds) bounds->push_back(in.position());
    return true;
}
}  // namespace

// length of an un-packed stream = tile-channels of its layer with more than `depth` atoms (:680-685): suffix sums
// of the histogram of lengths, once for all 6K streams
std::vector<size_t> expected_sizes(const std::vector<uint16_t>& lengths, int K) {
    std::vector<size_t> expect_of(static_cast<size_t>(3 * K), 0);
    std::vector<size_t> hist(static_cast<size_t>(3) * 65536, 0);
    for (size_t t = 0; t < lengths.size() / 3; ++t)
        for (size_t layer = 0; layer < 3; ++layer) ++hist[layer * 65536 + lengths[3 * t + layer]];
    for (size_t layer = 0; layer < 3; ++layer) {
        size_t above = 0;
        for (int v = 65535; v > K; --v) above += hist[layer * 65536 + static_cast<size_t>(v)];
        for (int depth = K - 1; depth >= 0; --depth) {
            above += hist[layer * 65536 + static_cast<size_t>(depth + 1)];
            expect_of[layer * static_cast<size_t>(K) + static_cast<size_t>(depth)] = above;
        }
    }
    std::vector<size_t> expect(static_cast<size_t>(6 * K), 0);
    for (int i = 0; i < 6 * K; ++i)
        expect[i] = expect_of[(static_cast<size_t>(i / 2) / K) * static_cast<size_t>(K) + static_cast<size_t>(i / 2) % K];
    return expect;
}

bool read_compressed_coded(const uint8_t* bytes, size_t nbytes, CodedStreams& s) { return parse_coded(bytes, nbytes, s, nullptr); }

// ------------------------------------------------------------------------------------------------
// The seek index.  The format chains a stream's first bit to the stream before it and a code's first bit to the code before it,
// and nothing else: with the bit of every stream's wrapper and of every interval-th code, every chunk of `interval` codes
// decodes on its own.  The index is a hint: plan_indexed_parse and the chunk decoders accept it only where the serial parser,
// started at bit 0, provably passes through every position it names with the same symbols.
//
// Blob, little-endian:   0 u32 magic "MPIX"  4 u32 version  8 u32 interval  12 u32 flags (1 = serial only)  16 u64 container bytes
//   24 u32 width  28 u32 height  32 u32 K  36 u32 block size  40 u32 streams (1 + 6K)  44 u32 0  48 u64 checkpoints in all
//   56 per stream, 64 bytes: u64 wrapper bit, end bit, coded symbols, expected symbols, first checkpoint, checkpoints;
//      u32 packed, mode, M, 0
//   then u64 per checkpoint
// Version 2 is that blob with version = 2, followed by the aux section: u64 aux entries in all, then -- stream behind stream in the
// blob's order, only for the streams that are run-length packed or step-0 coefficient streams -- 16 bytes per checkpoint:
//   u64 out (expanded symbols in front of the checkpoint), u64 prev | dc << 16 | state << 32 (IndexAux; the other bits zero)
// ------------------------------------------------------------------------------------------------
namespace {
constexpr uint32_t kIndexMagic = 0x5849504Du, kIndexVersion = 1, kIndexVersionExpanded = 2;
constexpr size_t kIndexHead = 56, kIndexStream = 64, kIndexAux = 16;

void put32(std::vector<uint8_t>& b, uint32_t v) { for (int k = 0; k < 4; ++k) b.push_back(static_cast<uint8_t>(v >> (8 * k))); }
void put64(std::vector<uint8_t>& b, uint64_t v) { for (int k = 0; k < 8; ++k) b.push_back(static_cast<uint8_t>(v >> (8 * k))); }
uint32_t get32(const uint8_t* p) { return p[0] | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24); }
uint64_t get64(const uint8_t* p) { return get32(p) | (static_cast<uint64_t>(get32(p + 4)) << 32); }

std::vector<uint8_t> index_blob(const ContainerIndex& x) {
    std::vector<uint8_t> b;
    uint64_t total = 0;
    for (const IndexStream& s : x.streams) total += s.checkpoints.size();
    b.reserve(kIndexHead + kIndexStream * x.streams.size() + 8 * total);
    put32(b, kIndexMagic); put32(b, x.version); put32(b, x.interval); put32(b, x.serial_only ? 1u : 0u);
    put64(b, x.nbytes);
    put32(b, static_cast<uint32_t>(x.width)); put32(b, static_cast<uint32_t>(x.height));
    put32(b, static_cast<uint32_t>(x.K)); put32(b, static_cast<uint32_t>(x.block_size));
    put32(b, static_cast<uint32_t>(x.streams.size())); put32(b, 0);
    put64(b, total);
    uint64_t first = 0;
    for (const IndexStream& s : x.streams) {
        put64(b, s.wrapper_bit); put64(b, s.end_bit); put64(b, s.n_coded); put64(b, s.expect);
        put64(b, first); put64(b, s.checkpoints.size());
        put32(b, s.packed); put32(b, s.mode); put32(b, s.m); put32(b, 0);
        first += s.checkpoints.size();
    }
    for (const IndexStream& s : x.streams)
        for (uint64_t c : s.checkpoints) put64(b, c);
    if (x.version == kIndexVersionExpanded) {
        uint64_t entries = 0;
        for (const IndexStream& s : x.streams) entries += s.aux.size();
        put64(b, entries);
        for (const IndexStream& s : x.streams)
            for (const IndexAux& a : s.aux) {
                put64(b, a.out);
                put64(b, static_cast<uint64_t>(a.prev) | (static_cast<uint64_t>(a.dc) << 16) | (static_cast<uint64_t>(a.state) << 32));
            }
    }
    return b;
}

// runLengthDecode's machine (rle_unpack; mp_unpack.hip's states) one coded symbol on: what it emits.  before: the coded symbol
// in front of v (looked at in states 1 and 2 only, where there is one)
struct RunMachine {
    unsigned state = 0;                                         // 0 fresh, 1 value, 2 count
    // the symbol emitted and how often
    void step(uint16_t v, uint16_t before, uint16_t* symbol, uint64_t* copies) {
        if (state == 2) {
            *symbol = before;
            *copies = v;
            state = 0;
        } else {
            *symbol = v;
            *copies = 1;
            state = state == 1 && v == before ? 2u : 1u;
        }
    }
};

// The aux entries of one stream: one linear pass over its coded symbols.  The blob is a pure function of (container, interval):
// nothing but the parsed symbols goes in
void index_aux_pass(const uint16_t* v, size_t n, uint32_t interval, bool packed, bool dc, std::vector<IndexAux>& aux) {
    aux.clear();
    aux.reserve((n + interval - 1) / interval);
    RunMachine run;
    uint64_t out = 0;
    uint32_t sum = 0;
    for (size_t i = 0; i < n; ++i) {
        if (i % interval == 0) {
            IndexAux a;
            a.out = out;
            a.prev = packed && i ? v[i - 1] : uint16_t(0);
            a.state = static_cast<uint8_t>(packed ? run.state : 0u);
            a.dc = dc ? static_cast<uint16_t>(sum) : uint16_t(0);
            aux.push_back(a);
        }
        uint16_t symbol = v[i];
        uint64_t copies = 1;
        if (packed) run.step(v[i], i ? v[i - 1] : uint16_t(0), &symbol, &copies);
        out += copies;
        if (dc) sum += static_cast<uint32_t>(copies) * static_cast<uint32_t>(zigzag_decode(symbol));
    }
}

void index_add_aux(ContainerIndex& x, const CodedStreams& s) {
    x.version = kIndexVersionExpanded;
    for (size_t j = 1; j < x.streams.size(); ++j) {
        IndexStream& is = x.streams[j];
        is.aux.clear();
        if (x.serial_only || !index_stream_has_aux(j, x.K, is.packed != 0)) continue;
        const std::vector<uint16_t>& v = s.codes[j - 1];
        index_aux_pass(v.data(), v.size(), x.interval, is.packed != 0, (j - 1) % (2 * static_cast<size_t>(x.K)) == 1, is.aux);
    }
}
}  // namespace

bool read_stream_wrapper(BitReader& in, bool has_flag, StreamWrapper& w) {
    w = StreamWrapper();
    if (has_flag && in.get(1) == 1) {
        w.packed = true;
        w.packed_size = in.get(32);
    }
    w.mode = static_cast<int>(in.get(1));
    if (w.mode == 0) {
        if (!read_huffman_codebook(in, w.cb)) return false;
    } else {
        w.m = static_cast<uint32_t>(in.get(16));
        if (w.m == 0) return false;
    }
    w.first_code_bit = in.position();
    return true;
}

bool build_container_index(const uint8_t* bytes, size_t nbytes, uint32_t interval, std::vector<uint8_t>& blob, bool expanded) {
    if (interval == 0) interval = kIndexIntervalDefault;
    CodedStreams s;
    std::vector<size_t> bounds;
    if (!parse_coded(bytes, nbytes, s, &bounds)) return false;
    const int n_streams = 6 * s.K + 1;
    ContainerIndex x;
    x.interval = interval;
    x.nbytes = nbytes;
    x.width = s.width; x.height = s.height; x.K = s.K; x.block_size = s.block_size;
    x.streams.resize(static_cast<size_t>(n_streams));
    // The positions inside a stream: its codes once more, one at a time, by the chunk decoders' own step.  Whatever that walk
    // cannot reproduce (codes longer than 32 bits; anything else would be a defect here) leaves an index that says
    // "serial only": still valid, never wrong.
    for (int j = 0; j < n_streams; ++j) {
        IndexStream& is = x.streams[static_cast<size_t>(j)];
        const std::vector<uint16_t>& want = j == 0 ? s.lengths : s.codes[static_cast<size_t>(j - 1)];
        is.wrapper_bit = bounds[static_cast<size_t>(j)];
        is.end_bit = bounds[static_cast<size_t>(j) + 1];
        is.n_coded = want.size();
        is.expect = j == 0 ? want.size() : s.expect[static_cast<size_t>(j - 1)];
        is.packed = j != 0 && s.packed[static_cast<size_t>(j - 1)];
        BitReader in(bytes, nbytes);
        in.set_position(is.wrapper_bit);
        StreamWrapper w;
        if (!read_stream_wrapper(in, j != 0, w)) { x.serial_only = true; continue; }
        is.mode = static_cast<uint32_t>(w.mode);
        is.m = w.m;
        if (x.serial_only) continue;
        bool same = true;
        uint32_t v = 0;
        for (size_t i = 0; i < want.size() && same; ++i) {
            if (i % interval == 0) is.checkpoints.push_back(in.position());
            if (w.mode == 0) same = huffman_step(w.cb, in, is.end_bit, &v) && v + 1u != w.cb.total && w.cb.table[v] == want[i];
            else same = golomb_step(w.m, in, is.end_bit, &v) && static_cast<uint16_t>(v) == want[i];
        }
        if (same && w.mode == 0) same = huffman_step(w.cb, in, is.end_bit, &v) && v + 1u == w.cb.total;
        if (!same || in.position() != is.end_bit) x.serial_only = true;
    }
    if (x.serial_only)
        for (IndexStream& is : x.streams) is.checkpoints.clear();
    if (expanded) index_add_aux(x, s);
    blob = index_blob(x);
    return true;
}

bool extend_container_index(const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes, std::vector<uint8_t>& blob) {
    ContainerIndex x;
    const bool readable = read_container_index(index, index_bytes, x);
    if (readable && x.version == kIndexVersionExpanded) {
        blob.assign(index, index + index_bytes);
        return true;
    }
    // the interval is the index's own word, whatever else of it is damaged; one that is no interval at all: the default
    uint32_t interval = readable ? x.interval : index && index_bytes >= 12 ? get32(index + 8) : 0u;
    if (interval < kIndexIntervalMin || interval > kIndexIntervalMax) interval = kIndexIntervalDefault;
    CodedStreams s;
    int route = 1;
    if (!read_compressed_coded_by_index(bytes, nbytes, index, index_bytes, s, &route)) return false;
    if (route != 0) return build_container_index(bytes, nbytes, interval, blob, true);
    // An accepted index: its positions and sizes are the serial parse's.  Mode and M are there for readers only and no decode
    // looks at them, so they are taken from the container's wrappers again
    for (size_t j = 0; j < x.streams.size(); ++j) {
        IndexStream& is = x.streams[j];
        BitReader in(bytes, nbytes);
        in.set_position(static_cast<size_t>(is.wrapper_bit));
        StreamWrapper w;
        if (!read_stream_wrapper(in, j != 0, w)) return build_container_index(bytes, nbytes, interval, blob, true);
        is.mode = static_cast<uint32_t>(w.mode);
        is.m = w.m;
    }
    index_add_aux(x, s);
    blob = index_blob(x);
    return true;
}

bool streams_match_lengths(const uint16_t* lengths, size_t tiles, int K, const unsigned long long* off) {
    const std::vector<size_t> expect = expected_sizes(std::vector<uint16_t>(lengths, lengths + 3 * tiles), K);
    for (int i = 0; i < 6 * K; ++i)
        if (off[i + 1] - off[i] != expect[static_cast<size_t>(i)]) return false;
    return true;
}

bool index_from_plan(uint32_t interval, size_t nbytes, int width, int height, int K, int block_size, size_t head_bits,
                     const StreamPlan* plans, const PlannedStream* streams, int n_streams, const uint64_t* checkpoints,
                     std::vector<uint8_t>& blob, bool expanded, const uint64_t* aux, size_t n_aux) {
    blob.clear();
    if (interval < kIndexIntervalMin || interval > kIndexIntervalMax || n_streams != 6 * K + 1) return false;
    ContainerIndex x;
    x.interval = interval;
    x.nbytes = nbytes;
    x.width = width; x.height = height; x.K = K; x.block_size = block_size;
    x.streams.resize(static_cast<size_t>(n_streams));
    if (expanded) x.version = kIndexVersionExpanded;
    size_t aux_at = 0;                                          // entries taken so far
    uint64_t bit = head_bits;
    const uint64_t* cp = checkpoints;
    for (int j = 0; j < n_streams; ++j) {
        const StreamPlan& p = plans[j];
        const PlannedStream& ps = streams[j];
        IndexStream& is = x.streams[static_cast<size_t>(j)];
        is.wrapper_bit = ps.first_code_bit - p.pre.bit_size();
        is.end_bit = ps.first_code_bit + p.payload_bits + p.post.bit_size();
        if (is.wrapper_bit != bit) return false;                // stream behind stream, the first behind the head
        bit = is.end_bit;
        is.n_coded = ps.eff_n;
        is.expect = ps.n;
        is.packed = j != 0 && ps.shorter;
        is.mode = static_cast<uint32_t>(p.mode);
        is.m = p.mode ? p.m : 0u;
        const size_t n_cp = static_cast<size_t>((ps.eff_n + interval - 1) / interval);
        // the code writer's positions: the first code's, then strictly forward, inside the stream's codes
        uint64_t before = ps.first_code_bit;
        for (size_t c = 0; c < n_cp; ++c) {
            if (c == 0 ? cp[c] != before : cp[c] <= before) return false;
            before = cp[c];
        }
        if (n_cp && before >= ps.first_code_bit + p.payload_bits) return false;
        is.checkpoints.assign(cp, cp + n_cp);
        cp += n_cp;
        if (!expanded || n_cp == 0 || !index_stream_has_aux(static_cast<size_t>(j), K, is.packed != 0)) continue;
        // The aux entries: an entry per checkpoint, and what read_container_index asks of a blob's own -- entry 0 fresh at
        // position 0, positions strictly forward and inside the stream, a state that exists, nothing in the unused bits, a
        // sum only where the stream is one of sums, an unpacked stream's positions its coded ones
        if (!aux || n_cp > n_aux - aux_at) return false;
        const bool dc = (j - 1) % (2 * K) == 1;
        is.aux.resize(n_cp);
        for (size_t c = 0; c < n_cp; ++c) {
            const uint64_t out = aux[2 * (aux_at + c)], word = aux[2 * (aux_at + c) + 1];
            IndexAux& e = is.aux[c];
            e.out = out;
            e.prev = static_cast<uint16_t>(word);
            e.dc = static_cast<uint16_t>(word >> 16);
            if ((word >> 32) > 2u) return false;
            e.state = static_cast<uint8_t>(word >> 32);
            if (c == 0 ? out != 0 || e.state != 0 || e.prev != 0 || e.dc != 0 : out <= is.aux[c - 1].out) return false;
            if (out > is.expect || (e.dc != 0 && !dc)) return false;
            if (!is.packed && (out != static_cast<uint64_t>(c) * interval || e.state != 0 || e.prev != 0)) return false;
        }
        aux_at += n_cp;
    }
    if ((bit + 7) / 8 != nbytes) return false;
    if (expanded && aux_at != n_aux) return false;                   // exactly the entries the plans imply
    blob = index_blob(x);
    return true;
}

bool read_container_index(const uint8_t* index, size_t index_bytes, ContainerIndex& x) {
    if (!index || index_bytes < kIndexHead) return false;
    const uint32_t version = get32(index + 4);
    if (get32(index) != kIndexMagic || (version != kIndexVersion && version != kIndexVersionExpanded)) return false;
    x = ContainerIndex();
    x.version = version;
    x.interval = get32(index + 8);
    const uint32_t flags = get32(index + 12);
    x.serial_only = (flags & 1u) != 0;
    x.nbytes = get64(index + 16);
    const uint32_t width = get32(index + 24), height = get32(index + 28), K = get32(index + 32), bs = get32(index + 36);
    const uint32_t n_streams = get32(index + 40);
    const uint64_t total = get64(index + 48);
    if (flags > 1u || get32(index + 44) != 0) return false;
    if (x.interval < kIndexIntervalMin || x.interval > kIndexIntervalMax) return false;
    if (K < 1 || K > 32 || bs < 1 || bs > 8 || width < 1 || height < 1 || width > 0x7FFFFFFFu || height > 0x7FFFFFFFu) return false;
    if (n_streams != 6 * K + 1) return false;
    const size_t fixed = kIndexHead + kIndexStream * n_streams;
    if (index_bytes < fixed || (index_bytes - fixed) % 8 != 0) return false;
    if (version == kIndexVersion ? total != (index_bytes - fixed) / 8 : total >= (index_bytes - fixed) / 8) return false;
    x.width = static_cast<int>(width); x.height = static_cast<int>(height); x.K = static_cast<int>(K); x.block_size = static_cast<int>(bs);
    x.streams.resize(n_streams);
    uint64_t first = 0;
    for (uint32_t j = 0; j < n_streams; ++j) {
        const uint8_t* r = index + kIndexHead + kIndexStream * j;
        IndexStream& is = x.streams[j];
        is.wrapper_bit = get64(r); is.end_bit = get64(r + 8); is.n_coded = get64(r + 16); is.expect = get64(r + 24);
        const uint64_t at = get64(r + 32), n_cp = get64(r + 40);
        is.packed = get32(r + 48); is.mode = get32(r + 52); is.m = get32(r + 56);
        if (at != first || n_cp > total - first || is.packed > 1u || is.mode > 1u || get32(r + 60) != 0) return false;
        is.checkpoints.resize(static_cast<size_t>(n_cp));
        for (uint64_t k = 0; k < n_cp; ++k) is.checkpoints[static_cast<size_t>(k)] = get64(index + fixed + 8 * (first + k));
        first += n_cp;
    }
    if (first != total) return false;
    if (version == kIndexVersion) return true;
    // The aux section: its size exact, an entry per checkpoint of every stream that has entries, and each stream's own order
    const uint8_t* at = index + fixed + 8 * static_cast<size_t>(total);          // total < (index_bytes - fixed) / 8: the count is inside
    const uint64_t entries = get64(at);
    const size_t room = index_bytes - fixed - 8 * static_cast<size_t>(total) - 8;
    if (room % kIndexAux != 0 || entries != room / kIndexAux) return false;
    uint64_t need = 0;
    for (uint32_t j = 1; j < n_streams; ++j)
        if (index_stream_has_aux(j, x.K, x.streams[j].packed != 0)) need += x.streams[j].checkpoints.size();
    if (need != entries) return false;
    at += 8;
    for (uint32_t j = 1; j < n_streams; ++j) {
        IndexStream& is = x.streams[j];
        if (!index_stream_has_aux(j, x.K, is.packed != 0)) continue;
        is.aux.resize(is.checkpoints.size());
        for (size_t k = 0; k < is.aux.size(); ++k, at += kIndexAux) {
            IndexAux& a = is.aux[k];
            const uint64_t word = get64(at + 8);
            a.out = get64(at);
            a.prev = static_cast<uint16_t>(word);
            a.dc = static_cast<uint16_t>(word >> 16);
            if ((word >> 32) > 2u) return false;                // the state, and the unused bits behind it
            a.state = static_cast<uint8_t>(word >> 32);
            if (k == 0 ? a.out != 0 || a.state != 0 || a.prev != 0 || a.dc != 0 : a.out <= is.aux[k - 1].out) return false;
            if (a.out > is.expect || (a.dc != 0 && (j - 1) % (2 * K) != 1)) return false;
            if (!is.packed && (a.out != static_cast<uint64_t>(k) * x.interval || a.state != 0 || a.prev != 0)) return false;
        }
    }
    return true;
}

bool plan_indexed_parse(const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes, IndexedPlan& plan, bool pooled) {
    ContainerIndex& x = plan.index;
    if (!read_container_index(index, index_bytes, x) || x.serial_only) return false;
    // the container's own header
    BitReader in(bytes, nbytes);
    int width, height, K, block_size;
    if (!read_header(in, &width, &height, &K, &block_size)) return false;
    if (x.nbytes != nbytes || x.width != width || x.height != height || x.K != K || x.block_size != block_size) return false;
    for (int ch = 0; ch < 3; ++ch)
        for (int i = 0; i < K; ++i) plan.quant[ch][i] = static_cast<uint16_t>(in.get(16));
    const size_t tiles = tile_count(width, height, block_size);
    if (tiles > (static_cast<size_t>(1) << 40) / 3) return false;
    plan.tiles = tiles;
    const uint64_t total_bits = 8 * static_cast<uint64_t>(nbytes);
    const size_t n_streams = x.streams.size();
    if (x.streams[0].wrapper_bit != in.position() || x.streams[0].n_coded != 3 * tiles || x.streams[0].packed) return false;
    plan.wrappers.resize(n_streams);
    // per stream: nothing here needs another stream's result (the index says where each wrapper begins)
    auto check_stream = [&](size_t j) -> bool {
        const IndexStream& is = x.streams[j];
        // positions: inside the container, strictly ordered, one checkpoint per `interval` codes, stream behind stream
        if (is.end_bit > total_bits || is.wrapper_bit >= is.end_bit) return false;
        if (j + 1 < n_streams && x.streams[j + 1].wrapper_bit != is.end_bit) return false;
        if (is.n_coded > is.end_bit - is.wrapper_bit) return false;            // every code takes at least one bit
        if (is.checkpoints.size() != (is.n_coded + x.interval - 1) / x.interval) return false;
        uint64_t before = is.wrapper_bit;
        for (uint64_t c : is.checkpoints) {
            if (c <= before || c >= is.end_bit) return false;
            before = c;
        }
        // the serial parser's own size checks
        if (j != 0) {
            if (is.expect > tiles) return false;
            if (is.packed ? is.n_coded - is.n_coded / 3 > is.expect : is.n_coded != is.expect) return false;
        }
        // the wrapper, from the container
        StreamWrapper& w = plan.wrappers[j];
        BitReader at(bytes, nbytes);
        at.set_position(static_cast<size_t>(is.wrapper_bit));
        if (!read_stream_wrapper(at, j != 0, w)) return false;
        if (w.packed != (is.packed != 0) || (w.packed && w.packed_size != is.n_coded)) return false;
        if (w.mode == 0 && w.cb.lut.empty()) return false;
        if (w.first_code_bit > is.end_bit) return false;
        if (!is.checkpoints.empty() && is.checkpoints[0] != w.first_code_bit) return false;
        if (is.checkpoints.empty()) {                           // a stream without codes: what must follow its wrapper, checked here
            uint16_t none;
            if (w.mode == 0 ? !huffman_decode_chunk(w.cb, bytes, nbytes, w.first_code_bit, static_cast<size_t>(is.end_bit), 0, true, &none)
                            : w.first_code_bit != is.end_bit)
                return false;
        }
        return true;
    };
    if (!pooled) {
        for (size_t j = 0; j < n_streams; ++j)
            if (!check_stream(j)) return false;
        return true;
    }
    std::vector<char> ok(n_streams, 0);
    parallel_jobs(static_cast<int>(n_streams), [&](int j) { ok[static_cast<size_t>(j)] = check_stream(static_cast<size_t>(j)) ? 1 : 0; });
    return std::find(ok.begin(), ok.end(), 0) == ok.end();
}

namespace {
// the acceptance rule whole: plan_indexed_parse, then every chunk by the chunk decoders; false = the index is not used
bool read_coded_by_index_alone(const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes, CodedStreams& out) {
    IndexedPlan plan;
    if (!plan_indexed_parse(bytes, nbytes, index, index_bytes, plan)) return false;
    const ContainerIndex& x = plan.index;
    const int K = x.K;
    auto decode_stream = [&](size_t j, std::vector<uint16_t>& dst) -> bool {
        const IndexStream& is = x.streams[j];
        const StreamWrapper& w = plan.wrappers[j];
        dst.assign(static_cast<size_t>(is.n_coded), 0);
        const size_t chunks = is.checkpoints.size();
        for (size_t c = 0; c < chunks; ++c) {
            const bool last = c + 1 == chunks;
            const size_t begin = static_cast<size_t>(is.checkpoints[c]);
            const size_t end = static_cast<size_t>(last ? is.end_bit : is.checkpoints[c + 1]);
            const size_t first = c * x.interval, count = std::min<size_t>(x.interval, dst.size() - first);
            if (w.mode == 0 ? !huffman_decode_chunk(w.cb, bytes, nbytes, begin, end, count, last, dst.data() + first)
                            : !golomb_decode_chunk(w.m, bytes, nbytes, begin, end, count, dst.data() + first))
                return false;
        }
        return true;
    };
    out = CodedStreams();
    out.width = x.width; out.height = x.height; out.K = K; out.block_size = x.block_size;
    std::memcpy(out.quant, plan.quant, sizeof(out.quant));
    if (!decode_stream(0, out.lengths)) return false;
    for (uint16_t length : out.lengths)
        if (length > K) return false;
    out.expect = expected_sizes(out.lengths, K);
    for (int i = 0; i < 6 * K; ++i)
        if (out.expect[i] != x.streams[static_cast<size_t>(i) + 1].expect) return false;
    out.codes.assign(static_cast<size_t>(6 * K), {});
    out.packed.assign(static_cast<size_t>(6 * K), 0);
    for (int i = 0; i < 6 * K; ++i) {
        out.packed[i] = static_cast<uint8_t>(x.streams[static_cast<size_t>(i) + 1].packed);
        if (!decode_stream(static_cast<size_t>(i) + 1, out.codes[i])) return false;
    }
    return true;
}
}  // namespace

bool read_compressed_coded_by_index(const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes, CodedStreams& out,
                                    int* route) {
    *route = 1;
    if (read_coded_by_index_alone(bytes, nbytes, index, index_bytes, out)) {
        *route = 0;
        return true;
    }
    out = CodedStreams();
    return read_compressed_coded(bytes, nbytes, out);
}

// ------------------------------------------------------------------------------------------------
// The seek index from a bit scan: the checkpoints without walking the codes one after another.  What
// mp_scan.hip's kernels compute per window, on the host: a step table (the code the serial parser's step finds at every bit), a map
// per segment (from every bit the first code start at or behind the segment's end, and the codes on the way), the chain through
// the segments from the stream's first bit, and the walk of every segment from its true entry that writes the checkpoints.
// Every loop is bounded by the window, the segment or the segment count; none iterates until nothing changes.
// ------------------------------------------------------------------------------------------------
namespace {
// a step: the code's bits in the low 24 | the pseudo-EOF | no code here (or it would pass the container's end)
constexpr uint32_t kStepDead = 0x80000000u, kStepEof = 0x40000000u, kStepLen = 0x00FFFFFFu;
// an exit, relative to the window's first bit: a code start at or behind the segment's end | the bit behind the pseudo-EOF | dead
constexpr uint32_t kExitDead = 0x80000000u, kExitEof = 0x40000000u, kExitPos = 0x3FFFFFFFu;
constexpr uint32_t kNoEntry = 0xFFFFFFFFu;

uint32_t scan_step(const StreamWrapper& w, BitReader& in, size_t p, size_t total) {
    in.set_position(p);
    uint32_t v = 0;
    if (w.mode == 0) {
        if (!huffman_step(w.cb, in, total, &v)) return kStepDead;
        return static_cast<uint32_t>(in.position() - p) | (v + 1u == w.cb.total ? kStepEof : 0u);
    }
    uint32_t ones = 0;                                          // the unary run, counted as far as the limit
    for (size_t q = p; ones < kScanUnaryLimit && q < total; q += 32) {
        in.set_position(q);
        const uint32_t window = in.peek32();
        if (window != 0xFFFFFFFFu) {
            ones += static_cast<uint32_t>(__builtin_clz(~window));
            break;
        }
        ones += 32;
    }
    if (ones >= kScanUnaryLimit) return kStepDead;
    in.set_position(p);
    if (!golomb_step(w.m, in, total, &v)) return kStepDead;
    return static_cast<uint32_t>(in.position() - p);
}
}  // namespace

bool scan_sizes_ok(uint32_t* segment_bits, uint32_t* window_bits) {
    if (*segment_bits == 0) *segment_bits = kScanSegmentDefault;
    if (*window_bits == 0) *window_bits = std::max(kScanWindowDefault, *segment_bits);
    if (*segment_bits < kScanSegmentMin || *segment_bits > kScanSegmentMax) return false;
    return *window_bits >= *segment_bits && *window_bits <= kScanWindowMax && *window_bits % *segment_bits == 0;
}

bool HostStreamScanner::scan(const StreamWrapper& w, uint64_t b0, uint64_t n, uint32_t interval, std::vector<uint64_t>& cps, uint64_t* end_bit) {
    const uint64_t total = 8 * static_cast<uint64_t>(nbytes);
    const bool golomb = w.mode == 1;
    if (!golomb && w.cb.lut.empty()) return false;              // codes longer than 32 bits: serial only
    cps.assign(static_cast<size_t>((n + interval - 1) / interval), 0);
    const uint32_t S = segment_bits;
    BitReader in(bytes, nbytes);
    std::vector<uint32_t> step, exit_of, entry;
    std::vector<uint16_t> count;
    std::vector<uint64_t> first;
    uint64_t pos = b0, ord = 0;                                 // the carry from window to window: a code start and its ordinal
    for (;;) {                                                  // every window moves pos on by its own length at least, or ends the stream
        if (golomb && ord == n) {
            *end_bit = pos;
            return true;
        }
        if (pos >= total) return false;
        const uint32_t wlen = static_cast<uint32_t>(std::min<uint64_t>(window_bits, total - pos));
        const uint32_t n_seg = (wlen + S - 1) / S;
        step.resize(wlen);
        for (uint32_t p = 0; p < wlen; ++p) step[p] = scan_step(w, in, static_cast<size_t>(pos + p), static_cast<size_t>(total));
        exit_of.resize(wlen);
        count.resize(wlen);
        for (uint32_t seg = 0; seg < n_seg; ++seg) {            // right to left: a position's path is its code and the next position's path
            const uint32_t lo = seg * S, hi = std::min(lo + S, wlen);
            for (uint32_t p = hi; p-- > lo;) {
                const uint32_t s = step[p], next = p + (s & kStepLen);
                if (s & kStepDead) { exit_of[p] = kExitDead; count[p] = 0; }
                else if (s & kStepEof) { exit_of[p] = kExitEof | next; count[p] = 0; }
                else if (next >= hi) { exit_of[p] = next; count[p] = 1; }
                else { exit_of[p] = exit_of[next]; count[p] = static_cast<uint16_t>(count[next] + 1u); }
            }
        }
        entry.assign(n_seg, kNoEntry);
        first.assign(n_seg, 0);
        uint64_t rel = 0, o = ord;
        uint32_t final_seg = kNoEntry;
        for (uint32_t it = 0; it < n_seg && rel < wlen; ++it) {  // every round enters a later segment
            const uint32_t seg = static_cast<uint32_t>(rel / S), e = exit_of[rel], c = count[rel];
            // a Golomb stream ends behind its n-th code, whatever the path behind that runs into: a dead path counts its codes too
            const bool ends_here = (e & kExitEof) || (golomb && o + c >= n);
            if ((e & kExitDead) && !ends_here) return false;
            entry[seg] = static_cast<uint32_t>(rel);
            first[seg] = o;
            if (ends_here) { final_seg = seg; break; }
            rel = e & kExitPos;
            o += c;
        }
        bool done = false;
        for (uint32_t seg = 0; seg < n_seg; ++seg) {
            if (entry[seg] == kNoEntry) continue;
            const uint32_t hi = std::min((seg + 1) * S, wlen);
            uint32_t p = entry[seg];
            uint64_t q = first[seg];
            for (uint32_t k = 0; k <= S; ++k) {                 // a code takes a bit at least: at most S codes begin in a segment
                if (golomb && q == n) {
                    if (seg == final_seg) { *end_bit = pos + p; done = true; }
                    break;
                }
                if (p >= hi) break;
                if (q < n && q % interval == 0) cps[static_cast<size_t>(q / interval)] = pos + p;
                const uint32_t s = step[p];
                if (s & kStepDead) return false;
                if (s & kStepEof) {
                    if (q != n) return false;                   // another count than the stream must hold
                    if (seg == final_seg) { *end_bit = pos + p + (s & kStepLen); done = true; }
                    break;
                }
                p += s & kStepLen;
                ++q;
            }
        }
        if (done) return true;
        if (final_seg != kNoEntry) return false;
        pos += rel;
        ord = o;
    }
}

bool propose_container_index(const uint8_t* bytes, size_t nbytes, uint32_t interval, StreamScanner& scanner, std::vector<uint8_t>& blob) {
    if (interval == 0) interval = kIndexIntervalDefault;
    BitReader in(bytes, nbytes);
    ContainerIndex x;
    if (!read_header(in, &x.width, &x.height, &x.K, &x.block_size)) return false;
    const int K = x.K;
    in.skip(static_cast<size_t>(16) * 3 * static_cast<size_t>(K));
    const size_t tiles = tile_count(x.width, x.height, x.block_size);
    if (tiles > (static_cast<size_t>(1) << 40) / 3) return false;
    const uint64_t total = 8 * static_cast<uint64_t>(nbytes);
    x.interval = interval;
    x.nbytes = nbytes;
    x.streams.resize(static_cast<size_t>(6 * K + 1));
    std::vector<size_t> expect;
    uint64_t at = in.position();
    for (size_t j = 0; j < x.streams.size(); ++j) {
        IndexStream& is = x.streams[j];
        if (at >= total) return false;
        BitReader r(bytes, nbytes);
        r.set_position(static_cast<size_t>(at));
        StreamWrapper w;
        if (!read_stream_wrapper(r, j != 0, w)) return false;
        const uint64_t want = j == 0 ? 3 * tiles : expect[j - 1];
        const uint64_t n = w.packed ? w.packed_size : want;
        if (w.packed && n - n / 3 > want) return false;
        if (n > total - w.first_code_bit) return false;         // every code takes a bit at least
        is.wrapper_bit = at;
        is.n_coded = n;
        is.expect = want;
        is.packed = w.packed ? 1u : 0u;
        is.mode = static_cast<uint32_t>(w.mode);
        is.m = w.m;
        if (!scanner.scan(w, w.first_code_bit, n, interval, is.checkpoints, &is.end_bit)) return false;
        if (is.end_bit > total || is.end_bit <= at) return false;
        if (j == 0) {                                           // the sizes of the 6K streams: the lengths, chunk by chunk
            std::vector<uint16_t> lengths(static_cast<size_t>(n), 0);
            const size_t chunks = is.checkpoints.size();
            for (size_t c = 0; c < chunks; ++c) {
                const bool last = c + 1 == chunks;
                const size_t begin = static_cast<size_t>(is.checkpoints[c]);
                const size_t end = static_cast<size_t>(last ? is.end_bit : is.checkpoints[c + 1]);
                const size_t from = c * interval, count = std::min<size_t>(interval, lengths.size() - from);
                if (w.mode == 0 ? !huffman_decode_chunk(w.cb, bytes, nbytes, begin, end, count, last, lengths.data() + from)
                                : !golomb_decode_chunk(w.m, bytes, nbytes, begin, end, count, lengths.data() + from))
                    return false;
            }
            for (uint16_t length : lengths)
                if (length > K) return false;
            expect = expected_sizes(lengths, K);
        }
        at = is.end_bit;
    }
    blob = index_blob(x);
    return true;
}

bool accept_proposed_index(const uint8_t* bytes, size_t nbytes, std::vector<uint8_t>& blob, bool expanded) {
    if (!expanded) return true;
    std::vector<uint8_t> v2;
    if (!extend_container_index(bytes, nbytes, blob.data(), blob.size(), v2)) return false;
    blob.swap(v2);
    return true;
}

bool scan_container_index(const uint8_t* bytes, size_t nbytes, uint32_t interval, bool expanded, uint32_t segment_bits, uint32_t window_bits,
                          std::vector<uint8_t>& blob, int* route) {
    *route = 0;
    HostStreamScanner scanner(bytes, nbytes, segment_bits, window_bits);
    CodedStreams s;
    // the scan proposes, the existing verifier decides: an accepted index is the serial parser's path
    if (propose_container_index(bytes, nbytes, interval, scanner, blob) && read_coded_by_index_alone(bytes, nbytes, blob.data(), blob.size(), s) &&
        accept_proposed_index(bytes, nbytes, blob, expanded))
        return true;
    *route = 1;
    blob.clear();
    return build_container_index(bytes, nbytes, interval, blob, expanded);
}

bool tile_window(int width, int height, int block_size, int x, int y, int w, int h, TileWindow& win) {
    if (width < 1 || height < 1 || block_size < 1 || x < 0 || y < 0 || w < 1 || h < 1 || w > width - x || h > height - y) return false;
    win.tiles_y = (height + block_size - 1) / block_size;
    win.tx0 = x / block_size;
    win.ty0 = y / block_size;
    win.tx1 = (x + w + block_size - 1) / block_size;
    win.ty1 = (y + h + block_size - 1) / block_size;
    win.t0 = static_cast<size_t>(win.tx0) * win.tiles_y + win.ty0;
    win.t1 = static_cast<size_t>(win.tx1 - 1) * win.tiles_y + win.ty1;
    return true;
}

void window_ranges(const uint16_t* lengths, int K, size_t t0, size_t t1, uint64_t* ranges) {
    for (int ch = 0; ch < 3; ++ch) {
        std::vector<uint64_t> hist(static_cast<size_t>(K) + 1, 0);
        auto write = [&](int which) {                           // tiles so far with more than i atoms: a suffix sum
            uint64_t above = 0;
            for (int i = K - 1; i >= 0; --i) {
                above += hist[static_cast<size_t>(i) + 1];
                ranges[2 * (static_cast<size_t>(ch) * K + i) + which] = above;
            }
        };
        for (size_t t = 0; t < t1; ++t) {
            if (t == t0) write(0);
            ++hist[std::min<size_t>(lengths[3 * t + ch], static_cast<size_t>(K))];
        }
        write(1);                                               // t0 < t1: write(0) has run
    }
}

void window_chunks(const IndexStream& is, uint32_t interval, uint64_t r0, uint64_t r1, size_t* c0, size_t* c1) {
    const size_t n = is.checkpoints.size();
    if (is.aux.size() != n || n == 0) {                         // by coded position
        *c0 = std::min<uint64_t>(r0 / interval, n);
        *c1 = std::min<uint64_t>((r1 + interval - 1) / interval, n);
        return;
    }
    *c0 = *c1 = 0;
    if (r0 >= r1) return;
    // out[] is strictly increasing from out[0] = 0 (read_container_index)
    const auto out_less = [](uint64_t r, const IndexAux& a) { return r < a.out; };
    *c0 = static_cast<size_t>(std::upper_bound(is.aux.begin(), is.aux.end(), r0, out_less) - is.aux.begin()) - 1;
    const auto less_out = [](const IndexAux& a, uint64_t r) { return a.out < r; };
    *c1 = static_cast<size_t>(std::lower_bound(is.aux.begin() + static_cast<std::ptrdiff_t>(*c0) + 1, is.aux.end(), r1, less_out) - is.aux.begin());
}

namespace {
// chunks [c0, c1) of stream j of a planned index into their places in dst (n_coded symbols; the rest stays zero and is never
// looked at), each accepted under the per-chunk rule
bool decode_index_chunks(const IndexedPlan& plan, const uint8_t* bytes, size_t nbytes, size_t j, size_t c0, size_t c1, std::vector<uint16_t>& dst) {
    const ContainerIndex& ix = plan.index;
    const IndexStream& is = ix.streams[j];
    const StreamWrapper& wr = plan.wrappers[j];
    dst.assign(static_cast<size_t>(is.n_coded), 0);
    const size_t chunks = is.checkpoints.size();
    for (size_t c = c0; c < c1 && c < chunks; ++c) {
        const bool last = c + 1 == chunks;
        const size_t begin = static_cast<size_t>(is.checkpoints[c]);
        const size_t end = static_cast<size_t>(last ? is.end_bit : is.checkpoints[c + 1]);
        const size_t first = c * ix.interval, count = std::min<size_t>(ix.interval, dst.size() - first);
        if (wr.mode == 0 ? !huffman_decode_chunk(wr.cb, bytes, nbytes, begin, end, count, last, dst.data() + first)
                         : !golomb_decode_chunk(wr.m, bytes, nbytes, begin, end, count, dst.data() + first))
            return false;
    }
    return true;
}
// The window route's first step: the lengths stream whole, no length above K, and the stream sizes they imply equal to the index's
bool lengths_by_index(const IndexedPlan& plan, const uint8_t* bytes, size_t nbytes, std::vector<uint16_t>& lengths, std::vector<size_t>& expect) {
    const ContainerIndex& ix = plan.index;
    if (!decode_index_chunks(plan, bytes, nbytes, 0, 0, ix.streams[0].checkpoints.size(), lengths)) return false;
    for (uint16_t length : lengths)
        if (length > ix.K) return false;
    expect = expected_sizes(lengths, ix.K);
    for (int i = 0; i < 6 * ix.K; ++i)
        if (expect[i] != ix.streams[static_cast<size_t>(i) + 1].expect) return false;
    return true;
}
}  // namespace

int window_chunks_by_index(const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes, int x, int y, int w, int h,
                           bool parse_all, std::vector<uint64_t>& chunks, int* route) {
    *route = 1;
    int width, height, K, block_size;
    if (!container_info(bytes, nbytes, &width, &height, &K, &block_size)) return 1;
    TileWindow win;
    if (!tile_window(width, height, block_size, x, y, w, h, win)) return 2;
    chunks.assign(12 * static_cast<size_t>(K), 0);
    IndexedPlan plan;
    if (!plan_indexed_parse(bytes, nbytes, index, index_bytes, plan)) return 0;
    const ContainerIndex& ix = plan.index;
    std::vector<uint16_t> lengths;
    std::vector<size_t> expect;
    if (!lengths_by_index(plan, bytes, nbytes, lengths, expect)) return 0;
    std::vector<uint64_t> ranges(6 * static_cast<size_t>(K), 0);
    window_ranges(lengths.data(), K, win.t0, win.t1, ranges.data());
    for (int i = 0; i < 6 * K; ++i) {
        const IndexStream& is = ix.streams[static_cast<size_t>(i) + 1];
        const bool whole = parse_all || (is.aux.empty() && (is.packed || i % (2 * K) == 1));
        size_t c0 = 0, c1 = is.checkpoints.size();
        if (!whole) window_chunks(is, ix.interval, ranges[2 * (i / 2)], ranges[2 * (i / 2) + 1], &c0, &c1);
        chunks[2 * static_cast<size_t>(i)] = c0;
        chunks[2 * static_cast<size_t>(i) + 1] = c1;
    }
    *route = 0;
    return 0;
}

int read_window_by_index(const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes, int x, int y, int w, int h,
                         bool parse_all, std::vector<uint16_t>& symbols, std::vector<uint64_t>& ranges, int* route, int steps) {
    *route = 1;
    int width, height, K, block_size;
    if (!container_info(bytes, nbytes, &width, &height, &K, &block_size)) return 1;
    TileWindow win;
    if (!tile_window(width, height, block_size, x, y, w, h, win)) return 2;
    ranges.assign(6 * static_cast<size_t>(K), 0);
    // a view: the lengths cut as truncate_container cuts them, to min(length, steps), once they have been checked; a stream of a step
    // at or above `kept` then owns no position
    const int kept = steps > 0 && steps < K ? steps : K;
    const auto cut_lengths = [&](std::vector<uint16_t>& lengths) {
        if (steps > 0)
            for (uint16_t& length : lengths) length = static_cast<uint16_t>(std::min<int>(length, steps));
    };
    // the slices [r0, r1) of expanded streams behind the lengths
    auto emit = [&](const std::vector<uint16_t>& lengths, const std::function<const uint16_t*(int)>& expanded) {
        size_t total = lengths.size();
        for (int p = 0; p < 3 * K; ++p) total += 2 * static_cast<size_t>(ranges[2 * p + 1] - ranges[2 * p]);
        symbols.clear();
        symbols.reserve(total);
        symbols.insert(symbols.end(), lengths.begin(), lengths.end());
        for (int i = 0; i < 6 * K; ++i) {
            const uint64_t r0 = ranges[2 * (i / 2)], r1 = ranges[2 * (i / 2) + 1];
            const uint16_t* src = expanded(i);
            if (r1 > r0) symbols.insert(symbols.end(), src + r0, src + r1);
        }
    };
    IndexedPlan plan;
    std::vector<uint16_t> lengths;
    std::vector<std::vector<uint16_t>> codes;
    auto by_index = [&]() -> bool {
        if (!plan_indexed_parse(bytes, nbytes, index, index_bytes, plan)) return false;
        const ContainerIndex& ix = plan.index;
        auto decode_chunks = [&](size_t j, size_t c0, size_t c1, std::vector<uint16_t>& dst) -> bool {
            return decode_index_chunks(plan, bytes, nbytes, j, c0, c1, dst);
        };
        // A stream with aux entries: chunks [c0, c1) alone, the expansion entered at checkpoint c0 in the state, at the position
        // and with the sum the index names, and held to what it names for checkpoint c1 (to the stream's size where the range
        // ends with the stream).  dst: `expect` symbols of which [out[c0], the exit position) are filled; [r0, r1) lies inside
        auto expand_window = [&](const IndexStream& is, int i, uint64_t r0, uint64_t r1, bool dc, std::vector<uint16_t>& dst) -> bool {
            size_t c0 = 0, c1 = 0;
            window_chunks(is, ix.interval, r0, r1, &c0, &c1);
            dst.assign(static_cast<size_t>(is.expect), 0);
            if (c0 == c1) return true;
            std::vector<uint16_t> v;
            if (!decode_chunks(static_cast<size_t>(i) + 1, c0, c1, v)) return false;
            const bool open_end = c1 == is.checkpoints.size();
            const size_t s0 = c0 * ix.interval, s1 = open_end ? v.size() : c1 * ix.interval;
            const IndexAux& in = is.aux[c0];
            const uint64_t limit = open_end ? is.expect : is.aux[c1].out;          // <= expect (read_container_index)
            RunMachine run;
            run.state = is.packed ? in.state : 0u;
            uint64_t at = in.out;
            uint32_t sum = in.dc;
            for (size_t k = s0; k < s1; ++k) {
                uint16_t symbol = v[k];
                uint64_t copies = 1;
                if (is.packed) run.step(v[k], k == s0 ? in.prev : v[k - 1], &symbol, &copies);
                if (copies > limit - at) return false;          // before anything of it is written
                for (uint64_t e = 0; e < copies; ++e) {
                    if (dc) {
                        sum += static_cast<uint32_t>(zigzag_decode(symbol));
                        dst[static_cast<size_t>(at + e)] = static_cast<uint16_t>(sum);
                    } else
                        dst[static_cast<size_t>(at + e)] = symbol;
                }
                at += copies;
            }
            if (at != limit) return false;                      // a count left dangling at the stream's end is dropped, as by rle_decode
            if (open_end) return true;
            const IndexAux& ex = is.aux[c1];
            return (is.packed ? run.state : 0u) == ex.state && (is.packed ? v[s1 - 1] : uint16_t(0)) == ex.prev &&
                   (dc ? static_cast<uint16_t>(sum) : uint16_t(0)) == ex.dc;
        };
        std::vector<size_t> expect;
        if (!lengths_by_index(plan, bytes, nbytes, lengths, expect)) return false;
        cut_lengths(lengths);                                   // behind the check against the index's (uncut) sizes
        window_ranges(lengths.data(), K, win.t0, win.t1, ranges.data());
        codes.assign(static_cast<size_t>(6 * K), {});
        for (int i = 0; i < 6 * K; ++i) {
            const IndexStream& is = ix.streams[static_cast<size_t>(i) + 1];
            const bool dc = i % (2 * K) == 1;
            if (!parse_all && (i % (2 * K)) / 2 >= kept) continue;   // a cut stream: never read
            const uint64_t r0 = ranges[2 * (i / 2)], r1 = ranges[2 * (i / 2) + 1];
            std::vector<uint16_t>& v = codes[i];
            if (!parse_all && !is.aux.empty()) {                // version 2: cut by expanded position
                if (!expand_window(is, i, r0, r1, dc, v)) return false;
                continue;
            }
            const bool whole = parse_all || is.packed || dc;
            size_t c0 = 0, c1 = is.checkpoints.size();
            if (!whole) window_chunks(is, ix.interval, r0, r1, &c0, &c1);
            if (!decode_chunks(static_cast<size_t>(i) + 1, c0, c1, v)) return false;
            if (is.packed) {                                    // whole: its size is what the lengths allow, or the serial route decides
                size_t expanded = 0;
                if (!rle_decoded_size(v.data(), v.size(), expect[i], &expanded) || expanded != expect[i]) return false;
                v = rle_decode(v.data(), v.size());
            }
            if (v.size() != expect[i]) return false;
            if (dc) {
                int32_t acc = 0;
                for (uint16_t& c : v) {
                    acc += zigzag_decode(c);
                    c = static_cast<uint16_t>(acc);
                }
            }
        }
        return true;
    };
    if (by_index()) {
        *route = 0;
        emit(lengths, [&](int i) { return codes[i].data(); });
        return 0;
    }
    Streams s;
    if (!read_compressed(bytes, nbytes, s)) return 1;
    cut_lengths(s.lengths);
    window_ranges(s.lengths.data(), K, win.t0, win.t1, ranges.data());
    emit(s.lengths, [&](int i) { return s.codes[i].data(); });
    return 0;
}

bool truncate_container(const uint8_t* bytes, size_t nbytes, int steps, std::vector<uint8_t>& out) {
    Streams s;
    if (!read_compressed(bytes, nbytes, s)) return false;
    const int K = s.K;
    for (uint16_t& length : s.lengths)
        if (static_cast<int>(length) > steps) length = static_cast<uint16_t>(steps);
    for (int ch = 0; ch < 3; ++ch)
        for (int i = std::max(steps, 0); i < K; ++i) {
            s.codes[static_cast<size_t>(2 * K * ch + 2 * i)].clear();
            s.codes[static_cast<size_t>(2 * K * ch + 2 * i + 1)].clear();
        }
    out = write_compressed(s);
    return true;
}

std::string transcode_rect_error(int width, int height, int block_size, int x, int y, int w, int h) {
    char text[200];
    TileWindow win;
    if (!tile_window(width, height, block_size, x, y, w, h, win)) {
        std::snprintf(text, sizeof text, "rectangle %dx%d at (%d, %d) is empty or not inside a frame of %dx%d", w, h, x, y, width, height);
        return text;
    }
    // inside the frame: x + w <= width and y + h <= height, nothing overflows
    const bool right = (x + w) % block_size == 0 || x + w == width, bottom = (y + h) % block_size == 0 || y + h == height;
    if (x % block_size != 0 || y % block_size != 0 || !right || !bottom) {
        std::snprintf(text, sizeof text, "rectangle %dx%d at (%d, %d) is not aligned to the %d-pixel tiles of a frame of %dx%d", w, h, x, y,
                      block_size, width, height);
        return text;
    }
    return std::string();
}

int transcode_container(const uint8_t* bytes, size_t nbytes, int x, int y, int w, int h, int steps, std::vector<uint8_t>& out) {
    Streams s;
    if (!read_compressed(bytes, nbytes, s)) return 1;
    const int K = s.K, m = steps > 0 && steps < K ? steps : K;
    for (uint16_t length : s.lengths)
        if (length > K) return 2;
    TileWindow win;
    if (!tile_window(s.width, s.height, s.block_size, x, y, w, h, win)) return 3;
    Streams cropped;
    cropped.width = w;
    cropped.height = h;
    cropped.K = K;
    cropped.block_size = s.block_size;
    std::memcpy(cropped.quant, s.quant, sizeof(s.quant));
    cropped.codes.assign(static_cast<size_t>(6 * K), {});
    const size_t tiles = s.lengths.size() / 3, nty = static_cast<size_t>(win.ty1 - win.ty0);
    cropped.lengths.reserve(3 * nty * static_cast<size_t>(win.tx1 - win.tx0));
    // One pass in the source's tile order, which is the new frame's too (both column-major): every stream pair has a cursor, and a
    // record moves over when its tile is in the grid and its step is kept.  read_compressed has held every stream to its size
    std::vector<size_t> cursor(static_cast<size_t>(3 * K), 0);
    for (size_t t = 0; t < tiles; ++t) {
        const size_t tx = t / static_cast<size_t>(win.tiles_y), ty = t % static_cast<size_t>(win.tiles_y);
        const bool inside = tx >= static_cast<size_t>(win.tx0) && tx < static_cast<size_t>(win.tx1) && ty >= static_cast<size_t>(win.ty0) &&
                            ty < static_cast<size_t>(win.ty1);
        for (int ch = 0; ch < 3; ++ch) {
            const int length = s.lengths[3 * t + static_cast<size_t>(ch)];
            if (inside) cropped.lengths.push_back(static_cast<uint16_t>(std::min(length, m)));
            for (int i = 0; i < length; ++i) {
                const size_t at = cursor[static_cast<size_t>(ch * K + i)]++;
                if (!inside || i >= m) continue;
                const size_t pair = static_cast<size_t>(2 * K * ch + 2 * i);
                cropped.codes[pair].push_back(s.codes[pair][at]);
                cropped.codes[pair + 1].push_back(s.codes[pair + 1][at]);
            }
        }
    }
    out = write_compressed(cropped);
    return 0;
}

namespace {
int compose_refuse(std::string& why, int verdict, const char* format, ...) __attribute__((format(printf, 3, 4)));
int compose_refuse(std::string& why, int verdict, const char* format, ...) {
    char text[320];
    va_list args;
    va_start(args, format);
    std::vsnprintf(text, sizeof text, format, args);
    va_end(args);
    why = text;
    return verdict;
}
}  // namespace

std::string compose_part_error(const ComposePart& part, int bs, int width, int height) {
    const std::string rect_error = transcode_rect_error(part.src_width, part.src_height, bs, part.x, part.y, part.w, part.h);
    if (!rect_error.empty()) return rect_error;
    char text[240];
    // inside its source: x + w and y + h do not overflow; the destination's sums are taken in 64 bits
    const long long right = static_cast<long long>(part.dx) + part.w, bottom = static_cast<long long>(part.dy) + part.h;
    if (part.dx < 0 || part.dy < 0 || part.dx % bs != 0 || part.dy % bs != 0) {
        std::snprintf(text, sizeof text, "(%d, %d) is not aligned to the %d-pixel tiles of the destination", part.dx, part.dy, bs);
        return text;
    }
    if (right > width || bottom > height) {
        std::snprintf(text, sizeof text, "%dx%d at (%d, %d) is not inside the destination of %dx%d", part.w, part.h, part.dx, part.dy, width, height);
        return text;
    }
    // a ragged tile carries its zero fill: it is the encode of pasted pixels only where the destination is ragged in the same way
    if ((part.x + part.w) % bs != 0 && right != width) {
        std::snprintf(text, sizeof text, "the ragged right edge at %d lands at %lld, not on the destination's edge %d", part.x + part.w, right, width);
        return text;
    }
    if ((part.y + part.h) % bs != 0 && bottom != height) {
        std::snprintf(text, sizeof text, "the ragged bottom edge at %d lands at %lld, not on the destination's edge %d", part.y + part.h, bottom,
                      height);
        return text;
    }
    return std::string();
}

int compose_plan(const uint8_t* const* bytes, const size_t* nbytes, int n_sources, const ComposePart* parts, int n_parts, int width, int height,
                 const ComposeDevice* device, ComposePlan& plan, std::string& why) {
    // 1. what needs no container
    if (!parts || (n_sources > 0 && (!bytes || !nbytes))) return compose_refuse(why, 2, "null argument");
    if (n_parts < 1) return compose_refuse(why, 2, "n_parts must be at least 1");
    if (width < 1 || height < 1) return compose_refuse(why, 2, "bad geometry");
    if (n_sources < 0) return compose_refuse(why, 2, "n_sources must not be negative");
    for (int s = 0; s < n_sources; ++s)
        if (!bytes[s]) return compose_refuse(why, 2, "source %d: null argument", s);
    for (int p = 0; p < n_parts; ++p) {
        if (parts[p].source < -1 || parts[p].source >= n_sources)
            return compose_refuse(why, 2, "part %d: source %d of %d", p, parts[p].source, n_sources);
        if (parts[p].source == -1 && !device) return compose_refuse(why, 2, "part %d: pixels need a device", p);
        if (parts[p].source == -1 && !parts[p].has_pixels) return compose_refuse(why, 2, "part %d: null argument", p);
    }
    if (n_sources == 0 && !device) return compose_refuse(why, 2, "n_sources must be at least 1: the host computes no tiles");
    // 2. every source's header, named by a part or not: a container holds one quantiser table
    plan.sources.assign(static_cast<size_t>(n_sources), {});
    for (int s = 0; s < n_sources; ++s) {
        ComposeSource& src = plan.sources[static_cast<size_t>(s)];
        if (!container_info(bytes[s], nbytes[s], &src.width, &src.height, &src.K, &src.block_size))
            return compose_refuse(why, 1, "source %d: Invalid input data", s);
        BitReader in(bytes[s], nbytes[s]);
        int skip[4];
        read_header(in, &skip[0], &skip[1], &skip[2], &skip[3]);
        for (int ch = 0; ch < 3; ++ch)
            for (int i = 0; i < src.K; ++i) src.quant[ch][i] = static_cast<uint16_t>(in.get(16));
        const ComposeSource& first = plan.sources[0];
        if (src.K != first.K) return compose_refuse(why, 2, "source %d: K %d, source 0 has K %d", s, src.K, first.K);
        if (src.block_size != first.block_size)
            return compose_refuse(why, 2, "source %d: block size %d, source 0 has block size %d", s, src.block_size, first.block_size);
        for (int ch = 0; ch < 3; ++ch)
            for (int i = 0; i < src.K; ++i)
                if (src.quant[ch][i] != first.quant[ch][i])
                    return compose_refuse(why, 2, "source %d: quantiser value %d of channel %d is %u, source 0 has %u", s, i, ch,
                                          static_cast<unsigned>(src.quant[ch][i]), static_cast<unsigned>(first.quant[ch][i]));
    }
    plan.K = n_sources > 0 ? plan.sources[0].K : device->K;
    plan.block_size = n_sources > 0 ? plan.sources[0].block_size : device->block_size;
    if (device && plan.K != device->K) return compose_refuse(why, 2, "container K %d, context K %d", plan.K, device->K);
    if (device && plan.block_size != device->block_size)
        return compose_refuse(why, 2, "stream block size %d, context block size %d", plan.block_size, device->block_size);
    // 3. every part's geometry
    const int bs = plan.block_size;
    const long long tiles_x = (static_cast<long long>(width) + bs - 1) / bs, tiles_y = (static_cast<long long>(height) + bs - 1) / bs;
    if (tiles_x * tiles_y >= (1LL << 31)) return compose_refuse(why, 2, "bad geometry");
    plan.tiles_x = static_cast<int>(tiles_x);
    plan.tiles_y = static_cast<int>(tiles_y);
    plan.parts.assign(parts, parts + n_parts);
    for (int p = 0; p < n_parts; ++p) {
        ComposePart& part = plan.parts[static_cast<size_t>(p)];
        int sw, sh;                                                 // the frame the rectangle is cut out of: pixels are a frame of their own
        if (part.source >= 0) {
            sw = plan.sources[static_cast<size_t>(part.source)].width;
            sh = plan.sources[static_cast<size_t>(part.source)].height;
            if (part.x == 0 && part.y == 0 && part.w == 0 && part.h == 0) {
                part.w = sw;
                part.h = sh;
            }
        } else {
            sw = part.w;
            sh = part.h;
        }
        part.src_width = sw;
        part.src_height = sh;
        const std::string geometry = compose_part_error(part, bs, width, height);
        if (!geometry.empty()) return compose_refuse(why, 2, "part %d: %s", p, geometry.c_str());
    }
    // 4. coverage: the owner of a tile is the last part whose grid holds it
    plan.owner.assign(static_cast<size_t>(tiles_x * tiles_y), -1);
    plan.owns.assign(static_cast<size_t>(n_parts), 0);
    for (int p = 0; p < n_parts; ++p) {
        const ComposePart& part = plan.parts[static_cast<size_t>(p)];
        const int ntx = (part.x + part.w + bs - 1) / bs - part.x / bs, nty = (part.y + part.h + bs - 1) / bs - part.y / bs;
        for (int i = 0; i < ntx; ++i)
            std::fill_n(plan.owner.begin() + (static_cast<long long>(part.dx / bs + i) * tiles_y + part.dy / bs), nty, p);
    }
    for (size_t t = 0; t < plan.owner.size(); ++t) {
        if (plan.owner[t] < 0)
            return compose_refuse(why, 2, "destination tile %zu (column %zu, row %zu) is covered by no part", t, t / static_cast<size_t>(tiles_y),
                                  t % static_cast<size_t>(tiles_y));
        plan.owns[static_cast<size_t>(plan.owner[t])] = 1;
    }
    return 0;
}

int compose_container(const uint8_t* const* bytes, const size_t* nbytes, int n_sources, const ComposePart* parts, int n_parts, int width, int height,
                      std::vector<uint8_t>& out, std::string& why) {
    ComposePlan plan;
    if (!bytes || !nbytes) return compose_refuse(why, 2, "null argument");
    if (const int verdict = compose_plan(bytes, nbytes, n_sources, parts, n_parts, width, height, nullptr, plan, why); verdict != 0) return verdict;
    // 5. the sources that owning parts name, as whole-frame records
    const int K = plan.K, bs = plan.block_size;
    struct Records {
        bool read = false;
        std::vector<uint16_t> counts;
        std::vector<uint32_t> choices;
    };
    std::vector<Records> records(static_cast<size_t>(n_sources));
    for (int p = 0; p < n_parts; ++p) {
        if (!plan.owns[static_cast<size_t>(p)]) continue;
        const int source = plan.parts[static_cast<size_t>(p)].source;
        Records& r = records[static_cast<size_t>(source)];
        if (r.read) continue;                                       // a lower part has named it, and it was sound
        Streams s;
        if (!read_compressed(bytes[source], nbytes[source], s)) return compose_refuse(why, 1, "part %d: Invalid input data", p);
        for (uint16_t length : s.lengths)
            if (length > K) return compose_refuse(why, 1, "part %d: Invalid bitstream", p);
        if (!disassemble_streams(s, r.counts, r.choices)) return compose_refuse(why, 1, "part %d: Invalid input data", p);
        r.read = true;
    }
    Streams made;
    made.width = width;
    made.height = height;
    made.K = K;
    made.block_size = bs;
    std::memcpy(made.quant, plan.sources[0].quant, sizeof(made.quant));
    made.codes.assign(static_cast<size_t>(6 * K), {});
    made.lengths.resize(3 * plan.owner.size());
    // the destination's tile order: every tile takes the counts and the records of its owner's source tile
    for (size_t t = 0; t < plan.owner.size(); ++t) {
        const ComposePart& part = plan.parts[static_cast<size_t>(plan.owner[t])];
        const Records& r = records[static_cast<size_t>(part.source)];
        const size_t tx = t / static_cast<size_t>(plan.tiles_y), ty = t % static_cast<size_t>(plan.tiles_y);
        const size_t src_tiles_y = static_cast<size_t>((part.src_height + bs - 1) / bs);
        const size_t from = (tx - static_cast<size_t>(part.dx / bs) + static_cast<size_t>(part.x / bs)) * src_tiles_y +
                            (ty - static_cast<size_t>(part.dy / bs) + static_cast<size_t>(part.y / bs));
        for (size_t ch = 0; ch < 3; ++ch) {
            const int length = r.counts[3 * from + ch];
            made.lengths[3 * t + ch] = static_cast<uint16_t>(length);
            for (int i = 0; i < length; ++i) {
                const uint32_t record = r.choices[(3 * from + ch) * static_cast<size_t>(K) + static_cast<size_t>(i)];
                const size_t pair = 2 * static_cast<size_t>(K) * ch + 2 * static_cast<size_t>(i);
                made.codes[pair].push_back(static_cast<uint16_t>(record & 0xFFFFu));
                made.codes[pair + 1].push_back(static_cast<uint16_t>(record >> 16));
            }
        }
    }
    out = write_compressed(made);
    return 0;
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
