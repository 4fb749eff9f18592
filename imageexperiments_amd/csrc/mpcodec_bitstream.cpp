// mpcodec_bitstream.cpp -- product: the C ABI's host-only entry points: the container writer and reader, the entropy stage on
// the host (mpc_assemble_*), and the bit-level primitives of CompressionLib/inc/BitBuffer.h as the entropy stage uses them.
#include <cstring>
#include <string>

#include "mpc_internal.h"

struct mpc_streams {
    mpc::CodedStreams s;            // `packed` and `expect` are empty in a handle of mpc_read_compressed
};

namespace {
uint8_t* give_bytes(const std::vector<uint8_t>& v, size_t* n) {
    uint8_t* p = static_cast<uint8_t*>(std::malloc(v.empty() ? 1 : v.size()));
    if (p && !v.empty()) std::memcpy(p, v.data(), v.size());
    *n = v.size();
    return p;
}
uint16_t* give_u16(const std::vector<uint16_t>& v, size_t* n) {
    uint16_t* p = static_cast<uint16_t*>(std::malloc(v.empty() ? 2 : v.size() * 2));
    if (p && !v.empty()) std::memcpy(p, v.data(), v.size() * 2);
    *n = v.size();
    return p;
}
// the arguments of the two symbol-stream entry points; MPC_OK = usable
mpc_status check_symbol_streams(int width, int height, int K, int block_size, const double* quant, const uint16_t* counts,
                                const uint16_t* symbols, const unsigned long long* stream_off, uint8_t** bytes, size_t* nbytes) {
    if (!quant || !counts || (!symbols && stream_off && stream_off[6 * K]) || !stream_off || !bytes || !nbytes || K < 1 || K > MPC_MAX_K ||
        block_size < 1 || width < 1 || height < 1)
        return fail(MPC_ERR_ARGUMENT, "bad argument");
    for (int s = 0; s < 6 * K; ++s)
        if (stream_off[s + 1] < stream_off[s]) return fail(MPC_ERR_ARGUMENT, "stream offsets must not decrease");
    return MPC_OK;
}
}  // namespace

extern "C" {

void mpc_free(void* p) { std::free(p); }

mpc_status mpc_write_compressed(int width, int height, int K, int block_size, const double* quant,
                                const uint16_t* lengths, size_t n_lengths, const uint16_t* const* codes,
                                const size_t* code_lengths, uint8_t** bytes, size_t* nbytes) {
    return guarded([&]() -> mpc_status {
    if (!quant || !bytes || !nbytes || (!lengths && n_lengths) || !codes || !code_lengths || K < 1 || K > MPC_MAX_K)
        return fail(MPC_ERR_ARGUMENT, "bad argument");
    mpc::Streams s;
    s.width = width; s.height = height; s.K = K; s.block_size = block_size;
    for (int ch = 0; ch < 3; ++ch)
        for (int i = 0; i < K; ++i) s.quant[ch][i] = mpc::header_quant(quant[ch * K + i]);
    s.lengths.assign(lengths, lengths + n_lengths);
    s.codes.resize(static_cast<size_t>(6 * K));
    for (int i = 0; i < 6 * K; ++i) s.codes[i].assign(codes[i], codes[i] + code_lengths[i]);
    *bytes = give_bytes(mpc::write_compressed(s), nbytes);
    return *bytes ? MPC_OK : fail(MPC_ERR_ALLOC, "out of memory");
    });
}

mpc_status mpc_assemble_streams(int width, int height, int K, int block_size, const double* quant,
                                const uint16_t* counts, const mpc_basis_choice* choices, uint8_t** bytes, size_t* nbytes) {
    return guarded([&]() -> mpc_status {
    if (!quant || !counts || !choices || !bytes || !nbytes || K < 1 || K > MPC_MAX_K || block_size < 1 || width < 1 || height < 1)
        return fail(MPC_ERR_ARGUMENT, "bad argument");
    *bytes = mpc::encode_records_malloc(width, height, K, block_size, quant, counts, reinterpret_cast<const uint32_t*>(choices), nbytes);
    return *bytes ? MPC_OK : fail(MPC_ERR_ALLOC, "out of memory");
    });
}

mpc_status mpc_assemble_planar_streams(int width, int height, int K, int block_size, const double* quant,
                                       const uint16_t* counts, const mpc_basis_choice* planar, uint8_t** bytes, size_t* nbytes) {
    return guarded([&]() -> mpc_status {
    if (!quant || !counts || !planar || !bytes || !nbytes || K < 1 || K > MPC_MAX_K || block_size < 1 || width < 1 || height < 1)
        return fail(MPC_ERR_ARGUMENT, "bad argument");
    *bytes = mpc::encode_planar_records_malloc(width, height, K, block_size, quant, counts, reinterpret_cast<const uint32_t*>(planar), nbytes);
    return *bytes ? MPC_OK : fail(MPC_ERR_ALLOC, "out of memory");
    });
}

mpc_status mpc_assemble_symbol_streams(int width, int height, int K, int block_size, const double* quant, const uint16_t* counts,
                                       const uint16_t* symbols, const unsigned long long* stream_off, uint8_t** bytes, size_t* nbytes) {
    return guarded([&]() -> mpc_status {
    if (const mpc_status bad = check_symbol_streams(width, height, K, block_size, quant, counts, symbols, stream_off, bytes, nbytes)) return bad;
    *bytes = mpc::encode_symbol_streams_malloc(width, height, K, block_size, quant, counts, symbols, stream_off, nbytes);
    return *bytes ? MPC_OK : fail(MPC_ERR_ALLOC, "out of memory");
    });
}

mpc_status mpc_assemble_symbol_streams_by_plan(int width, int height, int K, int block_size, const double* quant, const uint16_t* counts,
                                               const uint16_t* symbols, const unsigned long long* stream_off, uint8_t** bytes, size_t* nbytes) {
    return guarded([&]() -> mpc_status {
    if (const mpc_status bad = check_symbol_streams(width, height, K, block_size, quant, counts, symbols, stream_off, bytes, nbytes)) return bad;
    *bytes = mpc::encode_symbol_streams_by_plan_malloc(width, height, K, block_size, quant, counts, symbols, stream_off, nbytes);
    return *bytes ? MPC_OK : fail(MPC_ERR_ALLOC, "out of memory or inconsistent plan");
    });
}

namespace {
mpc_status assemble_by_plan_indexed(int width, int height, int K, int block_size, const double* quant, const uint16_t* counts,
                                    const uint16_t* symbols, const unsigned long long* stream_off, int interval, unsigned flags,
                                    uint8_t** bytes, size_t* nbytes, uint8_t** index, size_t* index_bytes) {
    return guarded([&]() -> mpc_status {
    if (!index || !index_bytes) return fail(MPC_ERR_ARGUMENT, "bad argument");
    if (const mpc_status bad = check_symbol_streams(width, height, K, block_size, quant, counts, symbols, stream_off, bytes, nbytes)) return bad;
    if (interval != 0 && (interval < static_cast<int>(mpc::kIndexIntervalMin) || interval > static_cast<int>(mpc::kIndexIntervalMax)))
        return fail(MPC_ERR_ARGUMENT, "interval %d: 0 or %u to %u", interval, mpc::kIndexIntervalMin, mpc::kIndexIntervalMax);
    if (flags & ~MPC_INDEX_EXPANDED) return fail(MPC_ERR_ARGUMENT, "flags 0x%x: MPC_INDEX_EXPANDED or 0", flags);
    *index = nullptr;
    *index_bytes = 0;
    std::vector<uint8_t> blob;
    uint8_t* container = mpc::encode_symbol_streams_by_plan_indexed_malloc(
        width, height, K, block_size, quant, counts, symbols, stream_off, interval ? static_cast<uint32_t>(interval) : mpc::kIndexIntervalDefault,
        nbytes, blob, (flags & MPC_INDEX_EXPANDED) != 0);
    if (!container) return fail(MPC_ERR_ALLOC, "out of memory or inconsistent plan");
    if (!blob.empty()) {
        *index = give_bytes(blob, index_bytes);
        if (!*index) {
            std::free(container);
            *index_bytes = 0;
            return fail(MPC_ERR_ALLOC, "out of memory");
        }
    }
    *bytes = container;
    return MPC_OK;
    });
}
}  // namespace

mpc_status mpc_assemble_symbol_streams_by_plan_indexed(int width, int height, int K, int block_size, const double* quant,
                                                       const uint16_t* counts, const uint16_t* symbols, const unsigned long long* stream_off,
                                                       int interval, uint8_t** bytes, size_t* nbytes, uint8_t** index, size_t* index_bytes) {
    return assemble_by_plan_indexed(width, height, K, block_size, quant, counts, symbols, stream_off, interval, 0, bytes, nbytes, index,
                                    index_bytes);
}

mpc_status mpc_assemble_symbol_streams_by_plan_indexed2(int width, int height, int K, int block_size, const double* quant,
                                                        const uint16_t* counts, const uint16_t* symbols, const unsigned long long* stream_off,
                                                        int interval, unsigned flags, uint8_t** bytes, size_t* nbytes, uint8_t** index,
                                                        size_t* index_bytes) {
    return assemble_by_plan_indexed(width, height, K, block_size, quant, counts, symbols, stream_off, interval, flags, bytes, nbytes, index,
                                    index_bytes);
}

mpc_status mpc_read_compressed(const uint8_t* bytes, size_t nbytes, mpc_streams** out) {
    return guarded([&]() -> mpc_status {
    if (!bytes || !out) return fail(MPC_ERR_ARGUMENT, "null argument");
    std::unique_ptr<mpc_streams> h(new mpc_streams);
    if (!mpc::read_compressed(bytes, nbytes, h->s)) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
    *out = h.release();
    return MPC_OK;
    });
}

mpc_status mpc_read_compressed_coded(const uint8_t* bytes, size_t nbytes, mpc_streams** out) {
    return guarded([&]() -> mpc_status {
    if (!bytes || !out) return fail(MPC_ERR_ARGUMENT, "null argument");
    std::unique_ptr<mpc_streams> h(new mpc_streams);
    if (!mpc::read_compressed_coded(bytes, nbytes, h->s)) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
    *out = h.release();
    return MPC_OK;
    });
}

int mpc_streams_packed(const mpc_streams* h, int index) {
    return h && index >= 0 && index < static_cast<int>(h->s.packed.size()) ? h->s.packed[index] : 0;
}

size_t mpc_streams_expected(const mpc_streams* h, int index) {
    if (!h || index < 0 || index >= static_cast<int>(h->s.codes.size())) return 0;
    return index < static_cast<int>(h->s.expect.size()) ? h->s.expect[index] : h->s.codes[index].size();
}

mpc_status mpc_container_info(const uint8_t* bytes, size_t nbytes, int* width, int* height, int* K, int* block_size) {
    if (!bytes || !width || !height || !K || !block_size) return fail(MPC_ERR_ARGUMENT, "null argument");
    if (!mpc::container_info(bytes, nbytes, width, height, K, block_size)) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
    return MPC_OK;
}

mpc_status mpc_streams_info(const mpc_streams* h, int* width, int* height, int* K, int* block_size) {
    if (!h) return fail(MPC_ERR_ARGUMENT, "null streams");
    if (width) *width = h->s.width;
    if (height) *height = h->s.height;
    if (K) *K = h->s.K;
    if (block_size) *block_size = h->s.block_size;
    return MPC_OK;
}

mpc_status mpc_streams_quant(const mpc_streams* h, uint16_t* quant) {
    if (!h || !quant) return fail(MPC_ERR_ARGUMENT, "null argument");
    for (int ch = 0; ch < 3; ++ch)
        for (int i = 0; i < h->s.K; ++i) quant[ch * h->s.K + i] = h->s.quant[ch][i];
    return MPC_OK;
}

size_t mpc_streams_length(const mpc_streams* h, int index) {
    if (!h) return 0;
    if (index < 0) return h->s.lengths.size();
    return index < static_cast<int>(h->s.codes.size()) ? h->s.codes[index].size() : 0;
}

mpc_status mpc_streams_copy(const mpc_streams* h, int index, uint16_t* dst) {
    if (!h || !dst) return fail(MPC_ERR_ARGUMENT, "null argument");
    const std::vector<uint16_t>* v = nullptr;
    if (index < 0) v = &h->s.lengths;
    else if (index < static_cast<int>(h->s.codes.size())) v = &h->s.codes[index];
    if (!v) return fail(MPC_ERR_ARGUMENT, "stream index %d out of range", index);
    if (!v->empty()) std::memcpy(dst, v->data(), v->size() * 2);
    return MPC_OK;
}

void mpc_streams_free(mpc_streams* h) { delete h; }

mpc_status mpc_huffman_encode(const uint16_t* data, size_t n, uint8_t** bytes, size_t* nbytes) {
    return guarded([&]() -> mpc_status {
    if ((!data && n) || !bytes || !nbytes) return fail(MPC_ERR_ARGUMENT, "null argument");
    mpc::BitWriter w;
    mpc::huffman_encode(data, n, w);
    *bytes = give_bytes(w.bytes(), nbytes);
    return *bytes ? MPC_OK : fail(MPC_ERR_ALLOC, "out of memory");
    });
}

mpc_status mpc_huffman_decode(const uint8_t* bytes, size_t nbytes, uint16_t** data, size_t* n) {
    return guarded([&]() -> mpc_status {
    if (!bytes || !data || !n) return fail(MPC_ERR_ARGUMENT, "null argument");
    mpc::BitReader r(bytes, nbytes);
    std::vector<uint16_t> out;
    if (!mpc::huffman_decode(r, out)) return fail(MPC_ERR_BITSTREAM, "Invalid bitstream");
    *data = give_u16(out, n);
    return *data ? MPC_OK : fail(MPC_ERR_ALLOC, "out of memory");
    });
}

mpc_status mpc_rle_encode(const uint16_t* data, size_t n, uint16_t** out, size_t* n_out) {
    return guarded([&]() -> mpc_status {
    if ((!data && n) || !out || !n_out) return fail(MPC_ERR_ARGUMENT, "null argument");
    *out = give_u16(mpc::rle_encode(data, n), n_out);
    return *out ? MPC_OK : fail(MPC_ERR_ALLOC, "out of memory");
    });
}

mpc_status mpc_rle_decode(const uint16_t* data, size_t n, uint16_t** out, size_t* n_out) {
    return guarded([&]() -> mpc_status {
    if ((!data && n) || !out || !n_out) return fail(MPC_ERR_ARGUMENT, "null argument");
    *out = give_u16(mpc::rle_decode(data, n), n_out);
    return *out ? MPC_OK : fail(MPC_ERR_ALLOC, "out of memory");
    });
}

// ---- bit-level primitives of CompressionLib/inc/BitBuffer.h, as the entropy stage uses them ----
uint32_t mpc_zigzag_encode(int32_t x) { return mpc::zigzag_encode(x); }
int32_t mpc_zigzag_decode(uint32_t x) { return mpc::zigzag_decode(x); }
uint32_t mpc_golomb_length(uint32_t value, uint32_t m) { return m ? mpc::golomb_length(value, m) : 0; }
uint32_t mpc_elias_fano_length(size_t n, uint16_t max_symbol) { return mpc::elias_fano_length(n, max_symbol); }

mpc_status mpc_bits_pack(const uint64_t* values, const int* widths, size_t n, uint8_t** bytes, size_t* nbytes, size_t* nbits) {
    return guarded([&]() -> mpc_status {
    if ((!values || !widths) && n) return fail(MPC_ERR_ARGUMENT, "null argument");
    if (!bytes || !nbytes || !nbits) return fail(MPC_ERR_ARGUMENT, "null argument");
    mpc::BitWriter w;
    for (size_t i = 0; i < n; ++i) {
        if (widths[i] < 0 || widths[i] > 64) return fail(MPC_ERR_ARGUMENT, "Invalid bit width");      // BitBuffer.cpp:80 throws here
        w.put(values[i], widths[i]);
    }
    *nbits = w.bit_size();
    *bytes = give_bytes(w.bytes(), nbytes);
    return *bytes ? MPC_OK : fail(MPC_ERR_ALLOC, "out of memory");
    });
}

mpc_status mpc_bits_unpack(const uint8_t* bytes, size_t nbytes, const int* widths, size_t n, uint64_t* values, size_t* remaining_bits) {
    if ((!bytes && nbytes) || ((!widths || !values) && n)) return fail(MPC_ERR_ARGUMENT, "null argument");
    mpc::BitReader r(bytes, nbytes);
    for (size_t i = 0; i < n; ++i) {
        if (widths[i] < 0 || widths[i] > 64) return fail(MPC_ERR_ARGUMENT, "Invalid bit width");
        values[i] = r.get(widths[i]);
    }
    if (remaining_bits) *remaining_bits = r.remaining();
    return MPC_OK;
}

mpc_status mpc_golomb_encode(const uint32_t* values, size_t n, uint32_t m, uint8_t** bytes, size_t* nbytes, size_t* nbits) {
    return guarded([&]() -> mpc_status {
    if ((!values && n) || !bytes || !nbytes || !nbits || m == 0) return fail(MPC_ERR_ARGUMENT, "bad argument");
    mpc::BitWriter w;
    for (size_t i = 0; i < n; ++i) mpc::golomb_write(values[i], m, w);
    *nbits = w.bit_size();
    *bytes = give_bytes(w.bytes(), nbytes);
    return *bytes ? MPC_OK : fail(MPC_ERR_ALLOC, "out of memory");
    });
}

mpc_status mpc_golomb_decode(const uint8_t* bytes, size_t nbytes, size_t n, uint32_t m, uint32_t* values, size_t* remaining_bits) {
    if ((!bytes && nbytes) || (!values && n) || m == 0) return fail(MPC_ERR_ARGUMENT, "bad argument");
    mpc::BitReader r(bytes, nbytes);
    for (size_t i = 0; i < n; ++i) values[i] = mpc::golomb_read(m, r);
    if (remaining_bits) *remaining_bits = r.remaining();
    return MPC_OK;
}

mpc_status mpc_elias_fano_encode(const uint16_t* sorted, size_t n, uint16_t max_symbol, uint8_t** bytes, size_t* nbytes, size_t* nbits) {
    return guarded([&]() -> mpc_status {
    if ((!sorted && n) || !bytes || !nbytes || !nbits) return fail(MPC_ERR_ARGUMENT, "null argument");
    for (size_t i = 0; i < n; ++i)
        if (sorted[i] > max_symbol || (i && sorted[i] < sorted[i - 1])) return fail(MPC_ERR_ARGUMENT, "sequence not sorted or beyond max_symbol");
    mpc::BitWriter w;
    mpc::elias_fano_write(sorted, n, max_symbol, w);
    *nbits = w.bit_size();
    *bytes = give_bytes(w.bytes(), nbytes);
    return *bytes ? MPC_OK : fail(MPC_ERR_ALLOC, "out of memory");
    });
}

mpc_status mpc_elias_fano_decode(const uint8_t* bytes, size_t nbytes, size_t n, uint16_t max_symbol, uint16_t* sorted, size_t* remaining_bits) {
    if ((!bytes && nbytes) || (!sorted && n)) return fail(MPC_ERR_ARGUMENT, "null argument");
    mpc::BitReader r(bytes, nbytes);
    if (!mpc::elias_fano_read(sorted, n, max_symbol, r)) return fail(MPC_ERR_BITSTREAM, "Invalid bitstream");
    if (remaining_bits) *remaining_bits = r.remaining();
    return MPC_OK;
}

}  // extern "C"
