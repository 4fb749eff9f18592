// host_bitstream.h -- product host code: the host's share of the entropy stage and the ".mn" container of the
// CompressionLib codec.  The device does whatever touches every symbol of an encode or a decode (mp_streams.hip,
// mp_entropy.hip, mp_unpack.hip); the host builds one code table per stream, writes the container's small pieces
// and parses containers -- and holds the whole stage once more, for frames the device stage cannot take and for
// the tests.  Every route must emit the reference's bytes exactly:
//   bit buffer, zigzag, Golomb, Elias-Fano     CompressionLib/src/BitBuffer.cpp, inc/BitBuffer.h
//   canonical Huffman + u16 run-length code     CompressionLib/src/Huffman.cpp
//   Huffman-or-Golomb choice, container layout  CompressionLib/src/CompressedImage.cpp:359-460, 635-707
// Huffman ties are broken the way the reference's only toolchain (MSVC STL) breaks them; see
// MsvcHashOrder in host_bitstream.cpp.
// Three sources behind this one header: host_bitstream.cpp (everything per symbol or per bit), host_container.cpp
// (the container, once per stream) and host_pool.cpp (the worker pool).
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

namespace mpc {

// The quantiser step as the container header carries it: writeCompressed stores static_cast<uint16_t>(quant)
// (CompressedImage.cpp:419-427) and readCompressed reads that back (:656-662), so a decoder reconstructs with these
// values, not with the encoder's doubles.  Every header writer and the distortion path (mpc_distortion_device) use it.
inline uint16_t header_quant(double q) { return static_cast<uint16_t>(q); }

class BitWriter {
public:
    void put(uint64_t value, int width);            // MSB first; width 0..64
    void append(const BitWriter& other);
    // put(code_of[s], length_of[s]) for every s in data[0..n), through a register accumulator (lengths 1..32)
    void put_codes(const uint16_t* data, size_t n, const uint32_t* code_of, const uint8_t* length_of, size_t total_bits);
    size_t bit_size() const { return nbits_; }
    const uint64_t* words() const { return words_.data(); }   // MSB-first, the last word zero-padded
    std::vector<uint8_t> bytes() const;             // zero-padded to a whole byte (BitBuffer::Save)
private:
    std::vector<uint64_t> words_;
    size_t nbits_ = 0;
};

class BitReader {
public:
    BitReader(const uint8_t* data, size_t nbytes) : p_(data), nbits_(8 * nbytes) {}
    // BitBuffer::ReadBits: the width is clipped to what remains; past the end it returns 0
    uint64_t get(int width);
    size_t remaining() const { return nbits_ - pos_; }
    // the next 32 bits left-aligned (zero beyond the end), without consuming them; skip() consumes
    uint32_t peek32() const;
    void skip(size_t bits) { pos_ += bits; }
    // for the decoders' fast loops (they read whole 64-bit words while at least eight bytes remain and fall back to get / peek32)
    const uint8_t* data() const { return p_; }
    size_t position() const { return pos_; }
    size_t size_bits() const { return nbits_; }
    void set_position(size_t bit) { pos_ = bit; }
private:
    const uint8_t* p_;
    size_t nbits_;
    size_t pos_ = 0;
};

inline uint32_t zigzag_encode(int32_t x) { return (static_cast<uint32_t>(x) << 1) ^ static_cast<uint32_t>(x >> 31); }
inline int32_t zigzag_decode(uint32_t x) { return static_cast<int32_t>((x >> 1) ^ static_cast<uint32_t>(-static_cast<int64_t>(x & 1))); }

uint32_t golomb_length(uint32_t value, uint32_t m);
void golomb_write(uint32_t value, uint32_t m, BitWriter& out);
uint32_t golomb_read(uint32_t m, BitReader& in);
void golomb_encode(const uint16_t* data, size_t n, uint32_t m, BitWriter& out);      // golomb_write of every symbol

// Elias-Fano code of a sorted sequence (BitBuffer.cpp:292-354): the Huffman symbol table uses it where it is shorter than raw
uint32_t elias_fano_length(size_t n, uint16_t max_symbol);
void elias_fano_write(const uint16_t* seq, size_t n, uint16_t max_symbol, BitWriter& out);
bool elias_fano_read(uint16_t* dst, size_t n, uint16_t max_symbol, BitReader& in);

void huffman_encode(const uint16_t* data, size_t n, BitWriter& out);
bool huffman_decode(BitReader& in, std::vector<uint16_t>& out);          // false = "Invalid bitstream"

// The table in front of a Huffman stream's codes, and what a decoder derives from it
struct HuffmanCodebook {
    static constexpr int kLutBits = 11;
    int max_length = 0;
    uint16_t total = 0;                             // entries; the last one is the pseudo-EOF
    std::vector<uint16_t> counts;                   // [max_length] codes of each length
    std::vector<uint16_t> table;                    // [total] entry -> symbol, in order of (length, symbol)
    std::vector<uint32_t> first_code, first_index;  // [max_length + 1] of each used length
    std::vector<uint32_t> lut;                      // [1 << kLutBits] by the next bits: (entry << 5) | length, 0 = no code this
                                                    // short; filled shortest length first.  Empty when max_length > 32
};
bool read_huffman_codebook(BitReader& in, HuffmanCodebook& cb);          // false = what huffman_decode refuses a table for
// One code at in's position, with huffman_decode's / golomb_read's decision, that ends at or before bit `end` (<= the data's
// bits); false = there is none.  *entry indexes cb.table (total - 1 = the pseudo-EOF); *value is not yet cut to 16 bits.
bool huffman_step(const HuffmanCodebook& cb, BitReader& in, size_t end, uint32_t* entry);
bool golomb_step(uint32_t m, BitReader& in, size_t end, uint32_t* value);
// `count` codes from bit `begin` that end exactly on bit `end`, none of them the pseudo-EOF; last: the pseudo-EOF follows them
// and it is what ends on `end`.  false = not so; out[0 .. count) may then hold anything
bool huffman_decode_chunk(const HuffmanCodebook& cb, const uint8_t* bytes, size_t nbytes, size_t begin, size_t end, size_t count,
                          bool last, uint16_t* out);
bool golomb_decode_chunk(uint32_t m, const uint8_t* bytes, size_t nbytes, size_t begin, size_t end, size_t count, uint16_t* out);

std::vector<uint16_t> rle_encode(const uint16_t* data, size_t n);
std::vector<uint16_t> rle_decode(const uint16_t* data, size_t n);
// the sizes rle_encode / rle_decode would produce, without producing them; rle_decoded_size: false once it exceeds `limit`
size_t rle_encoded_size(const uint16_t* data, size_t n);
bool rle_decoded_size(const uint16_t* data, size_t n, size_t limit, size_t* size);

void write_huffman_or_golomb(const uint16_t* data, size_t n, BitWriter& out);
bool read_huffman_or_golomb(BitReader& in, size_t length, std::vector<uint16_t>& out);

struct Streams {
    int width = 0, height = 0, K = 0, block_size = 0;
    uint16_t quant[3][32] = {};
    std::vector<uint16_t> lengths;                  // 3 per tile, x-outer / y-inner tile order
    std::vector<std::vector<uint16_t>> codes;       // [6K]: codes[2K*ch + 2i] deltaId, [+1] intCoeff of step i
};

// writeCompressed: codes are taken as the encoder holds them (DC coefficients not yet differenced)
std::vector<uint8_t> write_compressed(const Streams& s);
// readCompressed: codes come back with the DC differencing undone; false = invalid data.  The decoder expands the streams on
// the device and calls this on one refusal path only (a wrong block size or a length above K, to learn whether the streams
// expand at all): it is the reference for what a decoder accepts (mpc_read_compressed, the host tests), and the decoder
// holds itself to its verdict.
bool read_compressed(const uint8_t* bytes, size_t nbytes, Streams& out);

// The streams as entropy-decoded: codes[i] still run-length packed where packed[i] (the container's flag), the three step-0
// coefficient streams (1, 2K + 1, 4K + 1) still difference coded; expect[i] = the symbols stream i must expand to.
struct CodedStreams : Streams {
    std::vector<uint8_t> packed;                    // [6K]
    std::vector<size_t> expect;                     // [6K]
};
// The serial half of read_compressed (which is this + run-length expansion + DC sums on the worker pool): uses no pool and no
// shared state, so several threads may parse containers side by side.  false = invalid data
bool read_compressed_coded(const uint8_t* bytes, size_t nbytes, CodedStreams& out);
// ---- seek index ("Seek index"): where every stream and every interval-th code of it begins ----
struct StreamWrapper {                              // what stands in front of a stream's codes
    bool packed = false;                            // the run-length flag (never set for the lengths stream, which has none)
    uint64_t packed_size = 0;
    int mode = 0;                                   // 0 = Huffman, 1 = Golomb
    uint32_t m = 0;
    HuffmanCodebook cb;
    size_t first_code_bit = 0;
};
// false = what the serial parser refuses at this point (a bad table, M = 0)
bool read_stream_wrapper(BitReader& in, bool has_flag, StreamWrapper& w);

// Index version 2: what the expansion behind the codes has reached at a checkpoint, for the streams whose coded positions are
// not their expanded positions (run-length packed) or whose symbols are prefix sums (the step-0 coefficient streams)
struct IndexAux {
    uint64_t out = 0;                               // expanded symbols emitted by the coded symbols in front of the checkpoint
    uint16_t prev = 0;                              // the coded symbol in front of it (0 at the stream's start and if not packed)
    uint16_t dc = 0;                                // step-0 coefficient stream: low 16 bits of the sum of zigzagDecode over those `out`
    uint8_t state = 0;                              // runLengthDecode's state the checkpoint's symbol is met in: 0 fresh, 1 value, 2 count
};
struct IndexStream {
    uint64_t wrapper_bit = 0, end_bit = 0, n_coded = 0, expect = 0;
    uint32_t packed = 0, mode = 0, m = 0;
    std::vector<uint64_t> checkpoints;              // bit of coded symbol j * interval
    std::vector<IndexAux> aux;                      // version 2, and only for a packed or step-0 coefficient stream: one per checkpoint
};
// stream j of 1 + 6K (the lengths stream first) has aux entries in a version-2 index
inline bool index_stream_has_aux(size_t j, int K, bool packed) { return j != 0 && (packed || (j - 1) % (2 * static_cast<size_t>(K)) == 1); }
struct ContainerIndex {
    uint32_t version = 1;
    uint32_t interval = 0;
    bool serial_only = false;                       // a Huffman table with codes longer than 32 bits: no checkpoints
    uint64_t nbytes = 0;
    int width = 0, height = 0, K = 0, block_size = 0;
    std::vector<IndexStream> streams;               // [1 + 6K], the lengths stream first
};
constexpr uint32_t kIndexIntervalMin = 32, kIndexIntervalMax = 65536, kIndexIntervalDefault = 128;
// One serial parse of the container, positions recorded; false = what read_compressed_coded refuses.  interval 0 = the default.
// expanded: version 2 (the aux section behind the checkpoints: one more linear pass over the packed and step-0 streams)
bool build_container_index(const uint8_t* bytes, size_t nbytes, uint32_t interval, std::vector<uint8_t>& blob, bool expanded = false);
// The version-2 blob build_container_index(..., interval of `index`, expanded) gives, from a version-1 index of this container:
// the coded streams by read_compressed_coded_by_index (no serial parse unless the index is refused), then the aux pass.  A
// version-2 index comes back as a copy.  false = what read_compressed_coded refuses, or not an index at all
bool extend_container_index(const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes, std::vector<uint8_t>& blob);
// the blob alone: magic, version, sizes; for version 2 the aux section's own consistency (count, out[0] = 0, strictly increasing,
// <= expect, j * interval for an unpacked stream, state <= 2, entry 0 fresh, unused bits zero).  Says nothing about any container
bool read_container_index(const uint8_t* index, size_t index_bytes, ContainerIndex& out);
// A stream's window [r0, r1) of expanded positions in chunks [*c0, *c1): by expanded position where the stream has aux entries (c0
// the last checkpoint at or in front of r0, c1 the first behind c0 at or behind r1, else all that follow; nothing if r0 == r1),
// by coded position otherwise
void window_chunks(const IndexStream& is, uint32_t interval, uint64_t r0, uint64_t r1, size_t* c0, size_t* c1);
// the chunk range read_window_by_index parses of each of the 6K streams (all chunks where it parses a stream whole): from the
// lengths stream alone.  Returns 0, 1 = not a container's header, 2 = the rectangle; *route = 1: the index is refused or the
// lengths are not what it says -- nothing is parsed by it, chunks[] all zero.  chunks[2 * i], [2 * i + 1] = c0, c1 of stream i
int window_chunks_by_index(const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes, int x, int y, int w, int h,
                           bool parse_all, std::vector<uint64_t>& chunks, int* route);
// An index checked against its container as far as the host can without decoding a code (the acceptance rule's first half):
// the wrappers read from the container, the tables built.  false = the index is not used.
struct IndexedPlan {
    ContainerIndex index;
    std::vector<StreamWrapper> wrappers;            // [1 + 6K]
    size_t tiles = 0;
    uint16_t quant[3][32] = {};
};
// pooled: the streams' wrappers are read on the worker pool (a caller with the machine to itself: a single frame)
bool plan_indexed_parse(const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes, IndexedPlan& plan,
                        bool pooled = false);
// what the lengths stream says the 6K streams expand to (read_compressed_coded's `expect`)
std::vector<size_t> expected_sizes(const std::vector<uint16_t>& lengths, int K);
// read_compressed_coded chunk by chunk from the index; *route = 0: the index was used, 1: it was refused and the serial parse
// gave the result.  Returns what read_compressed_coded returns, `out` what it gives.
bool read_compressed_coded_by_index(const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes, CodedStreams& out,
                                    int* route);

// ---- the seek index without a serial parse ("Seek index from a bit scan") ----
// Which code begins at bit p of a stream, and how long it is, depends on the bits at p and the stream's table alone (huffman_step /
// golomb_step with the container's end as the required end).  Evaluated at every bit of a window, the serial parse is a walk along
// p -> p + len(p), which composes segment by segment: the checkpoints come out without walking the codes one after another.
constexpr uint32_t kScanSegmentDefault = 256, kScanWindowDefault = 1u << 22;
constexpr uint32_t kScanSegmentMin = 32, kScanSegmentMax = 1u << 15, kScanWindowMax = 1u << 26;
// A Golomb code whose unary run reaches this many bits is "no code here" to the scan (no encoder writes one: a symbol has 16 bits);
// it bounds the step of a lane on the device.  The scan then gives up and the serial builder answers
constexpr uint32_t kScanUnaryLimit = 1u << 16;
// 0 = the default; true = a segment of 32 ... 32768 bits and a window of whole segments, at most 2^26 bits
bool scan_sizes_ok(uint32_t* segment_bits, uint32_t* window_bits);
// One stream's checkpoints: from bit b0 the codes of a stream that has `n` of them (Huffman: the pseudo-EOF must follow exactly n;
// Golomb: the stream ends behind the n-th).  cps gets the bit of code j * interval for j * interval < n, *end_bit the bit behind
// the stream.  false = the scan gives up on this stream (a dead chain, another count).  n <= the bits behind b0 is the caller's check
struct StreamScanner {
    virtual ~StreamScanner() {}
    virtual bool scan(const StreamWrapper& w, uint64_t b0, uint64_t n, uint32_t interval, std::vector<uint64_t>& cps, uint64_t* end_bit) = 0;
};
// The host's scanner: step table, segment maps, chain and emit over windows of window_bits, as mp_scan.hip's kernels do them
struct HostStreamScanner : StreamScanner {
    const uint8_t* bytes;
    size_t nbytes;
    uint32_t segment_bits, window_bits;
    HostStreamScanner(const uint8_t* b, size_t n, uint32_t segment, uint32_t window) : bytes(b), nbytes(n), segment_bits(segment), window_bits(window) {}
    bool scan(const StreamWrapper& w, uint64_t b0, uint64_t n, uint32_t interval, std::vector<uint64_t>& cps, uint64_t* end_bit) override;
};
// The version-1 blob of the container from the scanner's checkpoints, stream behind stream in container order (the wrappers by
// read_stream_wrapper, the sizes of streams 1 ... 6K from the lengths stream decoded chunk by chunk from its fresh checkpoints).
// false = the scan gives up (the give-up rule); the blob is a proposal: nothing has verified it yet
bool propose_container_index(const uint8_t* bytes, size_t nbytes, uint32_t interval, StreamScanner& scanner, std::vector<uint8_t>& blob);
// build_container_index(bytes, nbytes, interval, blob, expanded) by the host scanner: the proposal, accepted only if
// read_compressed_coded_by_index takes route 0 with it (then it is the serial parser's path: the blob the serial builder makes);
// *route = 0.  Otherwise *route = 1 and the serial builder's result and verdict
bool scan_container_index(const uint8_t* bytes, size_t nbytes, uint32_t interval, bool expanded, uint32_t segment_bits, uint32_t window_bits,
                          std::vector<uint8_t>& blob, int* route);
// an accepted version-1 proposal in the version asked for: expanded = through extend_container_index.  false = it refuses
bool accept_proposed_index(const uint8_t* bytes, size_t nbytes, std::vector<uint8_t>& blob, bool expanded);

// ---- a pixel rectangle of a frame through the index ("Decoder: regions") ----
// The tiles a rectangle touches: the grid [tx0, tx1) x [ty0, ty1), inside the contiguous tile range [t0, t1) of the streams' order
// (t = tx * tiles_y + ty).  false = the rectangle is empty or not inside the frame
struct TileWindow {
    int tx0 = 0, ty0 = 0, tx1 = 0, ty1 = 0, tiles_y = 0;
    size_t t0 = 0, t1 = 0;
};
bool tile_window(int width, int height, int block_size, int x, int y, int w, int h, TileWindow& win);
// ranges[2 * (ch * K + i)], [+ 1]: the tiles in front of t0 / of t1 whose length, cut to K, exceeds step i -- the positions the
// window owns in the two streams of that pair.  lengths[3 * tiles]
void window_ranges(const uint16_t* lengths, int K, size_t t0, size_t t1, uint64_t* ranges);
// What the device's windowed parse computes, on the host: the lengths whole, then of every one of the 6K streams the EXPANDED symbols
// [r0, r1) (run lengths undone, step-0 coefficients summed), back to back.  Of a stream that is neither packed nor a step-0
// coefficient stream only the chunks that hold [r0, r1) are decoded, unless parse_all.  A packed or step-0 stream is decoded whole
// with a version-1 index; with version 2 (and not parse_all) only its chunks [c0, c1) of window_chunks, the expansion entered with
// aux entry c0 and held to aux entry c1 (position, state, the symbol in front, the DC sum; the stream's size where c1 is its end).
// *route = 0: by the index; 1: the index was refused (plan_indexed_parse, a chunk, the lengths, a packed stream's size, an
// end-of-range check) and read_compressed gave the result.
// Returns 0, 1 = invalid data (read_compressed's verdict), 2 = the rectangle is empty or not inside the frame
// steps > 0 (a view, "Decoder: views"): the windowed parse of truncate_container(bytes, steps) from this container and its own
// index.  The lengths stream is parsed whole and held to the index's sizes UNCUT; behind that check the lengths are cut to
// min(length, steps), so a stream of a step at or above `steps` owns no position (r0 = r1 = 0) and is never read -- unless
// parse_all, which parses and checks every stream and still emits nothing of the cut ones.  The lengths returned are the cut ones
int read_window_by_index(const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes, int x, int y, int w, int h,
                         bool parse_all, std::vector<uint16_t>& symbols, std::vector<uint64_t>& ranges, int* route, int steps = 0);

// ---- the first `steps` records of every tile-channel ("Decoder: views") ----
// The container is layered by pursuit step: a tile-channel has step i exactly when its length exceeds i, so the container of the
// same frame pursued for `steps` steps only is the parsed one with every length set to min(length, steps), the streams of steps
// below `steps` as they are (the same symbols) and the streams of steps at or above it empty; header, K and quantiser table kept,
// written by the one host coder (write_compressed).  steps >= K: the parsed container coded again.  false = read_compressed
// refuses the input.  steps >= 1 is the caller's to check
bool truncate_container(const uint8_t* bytes, size_t nbytes, int steps, std::vector<uint8_t>& out);

// ---- transcode: a view of a container as a container (include/mpcodec.h, "transcode"; DESIGN.md section 4, "Transcode") ----
// The container of the rectangle (x, y, w, h) of the frame, cut to its first `steps` steps (0 or above K: every step), from the
// source's symbols alone: tile (tx - tx0) * nty + (ty - ty0) of the new frame takes the first min(length, steps) records of tile
// tx * tiles_y + ty; the streams are assembled in the new order and written by the one host coder (write_compressed), which
// difference codes the step-0 coefficients from zero again and chooses packed-or-not and Huffman-or-Golomb again.  Header: w x h, the
// source's K, block size and quantiser steps.  No dictionary is involved: a record outside its dynamic dictionary is carried over.
// Returns 0, 1 = read_compressed refuses the input, 2 = a length above K, 3 = the rectangle is empty or not inside the frame.
// That the rectangle is tile aligned (transcode_rect_error) is the caller's to check: only then is the result the encode of the crop
int transcode_container(const uint8_t* bytes, size_t nbytes, int x, int y, int w, int h, int steps, std::vector<uint8_t>& out);
// empty, or why (x, y, w, h) cannot be transcoded out of a frame of width x height in tiles of block_size: it is empty or not inside
// the frame; x or y is no multiple of block_size; x + w (y + h) is neither a multiple of block_size nor the frame's width (height)
std::string transcode_rect_error(int width, int height, int block_size, int x, int y, int w, int h);

// ---- compose: a container from rectangles of containers (include/mpcodec.h, "compose"; DESIGN.md section 4, "Compose") ----
// The inverse of the transcode: destination tile (dtx0 + i) * tiles_y + (dty0 + j) takes the counts and records of its owner's source
// tile (stx0 + i) * src_tiles_y + (sty0 + j), the owner being the last part whose destination grid holds the tile.
struct ComposePart {
    int source = 0;                 // >= 0: (x, y, w, h) is a rectangle of container `source`, (0, 0, 0, 0) = all of it; -1: w x h pixels
    int x = 0, y = 0, w = 0, h = 0;
    int dx = 0, dy = 0;             // where the rectangle's top-left lands in the destination
    bool has_pixels = false;        // source == -1: the caller gave a pointer
    int src_width = 0, src_height = 0;      // compose_plan: the frame the rectangle is cut out of; for pixels w x h
};
struct ComposeSource {
    int width = 0, height = 0, K = 0, block_size = 0;
    uint16_t quant[3][32] = {};
};
struct ComposeDevice {              // the device route: pixel parts are legal, and K and block size must be these
    int K = 0, block_size = 0;
};
struct ComposePlan {
    int K = 0, block_size = 0, tiles_x = 0, tiles_y = 0;
    std::vector<ComposeSource> sources;
    std::vector<ComposePart> parts;         // rectangles resolved
    std::vector<int32_t> owner;             // per destination tile, in the destination's tile order
    std::vector<char> owns;                 // per part: it owns at least one tile
};
// empty, or why `part` (rectangle resolved, src_width x src_height set) cannot be placed into a width x height destination in tiles of
// bs: check 3 of mpc_compose_container
std::string compose_part_error(const ComposePart& part, int bs, int width, int height);
// Checks 1 to 4 of mpc_compose_container in their order and the owner map.  device: null for the host definition (a pixel part and
// n_sources == 0 are refused), else pixel parts are legal, K and block size are the device's where there is no source, and sources
// that have another K or block size are refused behind the header checks.  Returns 0, 1 = MPC_ERR_BITSTREAM, 2 = MPC_ERR_ARGUMENT
// with the text in `why`
int compose_plan(const uint8_t* const* bytes, const size_t* nbytes, int n_sources, const ComposePart* parts, int n_parts, int width, int height,
                 const ComposeDevice* device, ComposePlan& plan, std::string& why);
// mpc_compose_container: the plan, then every source an owning part names through read_compressed, the records placed in the
// destination's tile order, write_compressed.  Verdicts as compose_plan's
int compose_container(const uint8_t* const* bytes, const size_t* nbytes, int n_sources, const ComposePart* parts, int n_parts, int width, int height,
                      std::vector<uint8_t>& out, std::string& why);

// The same index from what an encoder holds when it has just written the container, without parsing anything: the plans of
// plan_stream, where each stream's codes begin, and the bit of every interval-th coded symbol as the code writer passed it.
struct StreamPlan;                                  // below
struct PlannedStream {                              // one per stream, the lengths stream first
    uint64_t first_code_bit = 0;                    // where the stream's codes begin in the container (behind its wrapper)
    uint64_t n = 0, eff_n = 0;                      // symbols as assembled; symbols that were coded (after run-length packing)
    bool shorter = false;                           // the run-length packed stream is what was coded
};
// checkpoints: stream behind stream, ceil(eff_n / interval) each (the blob's own order).  The blob build_container_index gives
// for that container, provided the streams hold what the lengths stream implies (streams_match_lengths) and no Huffman code is
// longer than 32 bits.  false = the positions contradict the plans (head_bits, stream behind stream, checkpoints in order);
// `blob` is then empty.
// expanded: index version 2, with aux (n_aux entries of two words, out then prev | dc << 16 | state << 32) the entries of the streams
// that have any (index_stream_has_aux), stream behind stream, ceil(eff_n / interval) each: the blob
// build_container_index(..., expanded) gives.  false as well where the entries contradict the plans: not exactly that many,
// out[0] != 0, out not strictly increasing or beyond the stream's size, a state above 2, out[c] != c * interval for a stream that
// is not packed (and whatever else read_container_index would refuse in the blob)
bool index_from_plan(uint32_t interval, size_t nbytes, int width, int height, int K, int block_size, size_t head_bits,
                     const StreamPlan* plans, const PlannedStream* streams, int n_streams, const uint64_t* checkpoints,
                     std::vector<uint8_t>& blob, bool expanded = false, const uint64_t* aux = nullptr, size_t n_aux = 0);
// every one of the 6K streams holds as many symbols as the lengths stream implies (expected_sizes): what the serial parser
// goes by.  lengths[3 * tiles], off[6K + 1]
bool streams_match_lengths(const uint16_t* lengths, size_t tiles, int K, const unsigned long long* off);

// the header alone; false = not a container read_compressed would accept the header of
bool container_info(const uint8_t* bytes, size_t nbytes, int* width, int* height, int* K, int* block_size);
// worker threads of the host stages (MPC_HOST_THREADS, else the machine's, at most 16)
int host_thread_count();

// The container from per-tile records in the reference's visiting order (tile t = tx*tiles_y + ty): counts[t*3+ch],
// choices[(t*3+ch)*K + i] = deltaId | intCoeff << 16 (encodeImage, CompressedImage.cpp:555-572, + writeCompressed), in a
// malloc'ed buffer (release with free); nullptr = out of memory.  What mpc_assemble_streams uses.
uint8_t* encode_records_malloc(int width, int height, int K, int block_size, const double* quant, const uint16_t* counts,
                               const uint32_t* choices, size_t* nbytes);
// same container from records in planar order, planar[(ch * K + i) * tiles + t]: every (channel, step) job then reads
// one contiguous run instead of one word per 12*K bytes (mpc_assemble_planar_streams)
uint8_t* encode_planar_records_malloc(int width, int height, int K, int block_size, const double* quant, const uint16_t* counts,
                                      const uint32_t* planar, size_t* nbytes);

// same container from streams assembled on the device (mp_streams.hip): symbols = codes[0] ++ codes[1] ++ ... (live symbols
// only, step-0 coefficients already difference coded), off[6K + 1] = stream boundaries in symbols
uint8_t* encode_symbol_streams_malloc(int width, int height, int K, int block_size, const double* quant, const uint16_t* counts,
                                      const uint16_t* symbols, const unsigned long long* off, size_t* nbytes);

// ---- the host's share of the entropy stage when the device does the per-symbol work (mp_entropy.hip) ----
struct StreamPlan {
    BitWriter pre;                   // what precedes the stream's codes: run-length flag (+ size), Huffman/Golomb bit, table or M
    BitWriter post;                  // what follows them: the pseudo-EOF code (Huffman)
    size_t payload_bits = 0;         // bits of the codes themselves
    int mode = 0;                    // 0 = Huffman, 1 = Golomb
    uint32_t m = 0;                  // Golomb parameter
    int max_code_length = 0;         // Huffman
    std::vector<uint32_t> entries;   // Huffman: (symbol, code, length) of every symbol that occurs
};
// One stream of the container from its statistics: n coded symbols (after run-length coding if `shorter`), `largest` of them,
// triples[3 * distinct] = (symbol, count, position of first appearance) in any order.  rle_flag: false for `lengths`.
void plan_stream(bool rle_flag, bool shorter, uint32_t rle_size, size_t n, uint32_t largest, const uint32_t* triples, size_t distinct,
                 StreamPlan& plan);
BitWriter container_head(int width, int height, int K, int block_size, const double* quant /*[3*K]*/);
// dst |= piece, MSB first, at bit_offset (dst: the container's bytes, dst_bytes of them writable)
void or_bits(uint8_t* dst, size_t dst_bytes, size_t bit_offset, const BitWriter& piece);
// body(0..n-1) on the entropy stage's worker pool
void parallel_jobs(int n, const std::function<void(int)>& body);
// the same on a second pool of at most `workers` threads (the calling thread included): copies that run beside the entropy stage
void parallel_io_jobs(int n, int workers, const std::function<void(int)>& body);

// encode_symbol_streams_malloc through plan_stream / or_bits, the device's share (statistics, code writing) done on the host
uint8_t* encode_symbol_streams_by_plan_malloc(int width, int height, int K, int block_size, const double* quant, const uint16_t* counts,
                                              const uint16_t* symbols, const unsigned long long* off, size_t* nbytes);

// The same container together with its seek index, the checkpoints recorded while the codes are written: this defines what
// the device's code kernel records (mp_entropy.hip).  Streams that do not match the lengths stream: the container alone,
// `index` empty.  A Huffman code longer than 32 bits: build_container_index of the finished container.  interval: 32 ... 65536.
// expanded: index version 2, the aux entries by index_aux_pass over the coded streams this route holds -- which defines what the
// device's pack pass and sum kernels compute
uint8_t* encode_symbol_streams_by_plan_indexed_malloc(int width, int height, int K, int block_size, const double* quant,
                                                      const uint16_t* counts, const uint16_t* symbols, const unsigned long long* off,
                                                      uint32_t interval, size_t* nbytes, std::vector<uint8_t>& index,
                                                      bool expanded = false);

// Inverse of encode_records_malloc's gathering: per-tile records in the reference's visiting order.  counts[3*tiles],
// choices[3*tiles*K] (deltaId | intCoeff << 16, zero beyond count).  false = streams inconsistent with `lengths`.
bool disassemble_streams(const Streams& s, std::vector<uint16_t>& counts, std::vector<uint32_t>& choices);
// same into caller-provided storage (3*tiles and 3*tiles*K elements); entries beyond a count are left untouched
bool disassemble_streams(const Streams& s, uint16_t* counts, uint32_t* choices);

}  // namespace mpc
