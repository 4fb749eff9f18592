// mpcodec_index.cpp -- product: the C ABI's host-only entry points of the seek index (host_container.cpp): build one, read one
// back, and the chunked parses on the host -- of a whole frame, of a pixel rectangle's window -- that define what the device parse
// (mp_parse.hip) computes.
#include <cstring>
#include <string>

#include "mpc_internal.h"

extern "C" {

mpc_status mpc_container_index(const uint8_t* bytes, size_t nbytes, int interval, uint8_t** index, size_t* index_bytes) {
    return guarded([&]() -> mpc_status {
        if (!bytes || !index || !index_bytes) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (interval != 0 && (interval < static_cast<int>(mpc::kIndexIntervalMin) || interval > static_cast<int>(mpc::kIndexIntervalMax)))
            return fail(MPC_ERR_ARGUMENT, "interval %d: 0 or %u to %u", interval, mpc::kIndexIntervalMin, mpc::kIndexIntervalMax);
        std::vector<uint8_t> blob;
        if (!mpc::build_container_index(bytes, nbytes, static_cast<uint32_t>(interval), blob)) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
        uint8_t* p = static_cast<uint8_t*>(std::malloc(blob.size()));
        if (!p) return fail(MPC_ERR_ALLOC, "out of memory");
        std::memcpy(p, blob.data(), blob.size());
        *index = p;
        *index_bytes = blob.size();
        return MPC_OK;
    });
}

namespace {
mpc_status give_blob(const std::vector<uint8_t>& blob, uint8_t** index, size_t* index_bytes) {
    uint8_t* p = static_cast<uint8_t*>(std::malloc(blob.empty() ? 1 : blob.size()));
    if (!p) return fail(MPC_ERR_ALLOC, "out of memory");
    if (!blob.empty()) std::memcpy(p, blob.data(), blob.size());
    *index = p;
    *index_bytes = blob.size();
    return MPC_OK;
}
}  // namespace

mpc_status mpc_container_index2(const uint8_t* bytes, size_t nbytes, int interval, unsigned flags, uint8_t** index, size_t* index_bytes) {
    return guarded([&]() -> mpc_status {
        if (!bytes || !index || !index_bytes) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (flags & ~MPC_INDEX_EXPANDED) return fail(MPC_ERR_ARGUMENT, "flags 0x%x", flags);
        if (interval != 0 && (interval < static_cast<int>(mpc::kIndexIntervalMin) || interval > static_cast<int>(mpc::kIndexIntervalMax)))
            return fail(MPC_ERR_ARGUMENT, "interval %d: 0 or %u to %u", interval, mpc::kIndexIntervalMin, mpc::kIndexIntervalMax);
        std::vector<uint8_t> blob;
        if (!mpc::build_container_index(bytes, nbytes, static_cast<uint32_t>(interval), blob, (flags & MPC_INDEX_EXPANDED) != 0))
            return fail(MPC_ERR_BITSTREAM, "Invalid input data");
        return give_blob(blob, index, index_bytes);
    });
}

mpc_status mpc_container_index_scan(const uint8_t* bytes, size_t nbytes, int interval, unsigned flags, int segment_bits, int window_bits,
                                    uint8_t** index, size_t* index_bytes, int* route) {
    return guarded([&]() -> mpc_status {
        if (!bytes || !index || !index_bytes || !route) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (flags & ~MPC_INDEX_EXPANDED) return fail(MPC_ERR_ARGUMENT, "flags 0x%x", flags);
        if (interval != 0 && (interval < static_cast<int>(mpc::kIndexIntervalMin) || interval > static_cast<int>(mpc::kIndexIntervalMax)))
            return fail(MPC_ERR_ARGUMENT, "interval %d: 0 or %u to %u", interval, mpc::kIndexIntervalMin, mpc::kIndexIntervalMax);
        uint32_t segment = segment_bits < 0 ? 1u : static_cast<uint32_t>(segment_bits), window = window_bits < 0 ? 1u : static_cast<uint32_t>(window_bits);
        if (!mpc::scan_sizes_ok(&segment, &window))
            return fail(MPC_ERR_ARGUMENT, "segment of %d bits, window of %d: 0, or a segment of %u to %u bits and a window of whole segments up to %u bits",
                        segment_bits, window_bits, mpc::kScanSegmentMin, mpc::kScanSegmentMax, mpc::kScanWindowMax);
        std::vector<uint8_t> blob;
        if (!mpc::scan_container_index(bytes, nbytes, static_cast<uint32_t>(interval), (flags & MPC_INDEX_EXPANDED) != 0, segment, window, blob, route))
            return fail(MPC_ERR_BITSTREAM, "Invalid input data");
        return give_blob(blob, index, index_bytes);
    });
}

mpc_status mpc_index_extend(const uint8_t* bytes, size_t nbytes, const uint8_t* index_v1, size_t index_v1_bytes, uint8_t** index,
                            size_t* index_bytes) {
    return guarded([&]() -> mpc_status {
        if (!bytes || !index_v1 || !index || !index_bytes) return fail(MPC_ERR_ARGUMENT, "null argument");
        std::vector<uint8_t> blob;
        if (!mpc::extend_container_index(bytes, nbytes, index_v1, index_v1_bytes, blob)) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
        return give_blob(blob, index, index_bytes);
    });
}

int mpc_index_version(const uint8_t* index, size_t index_bytes) {
    mpc::ContainerIndex x;
    try {
        return index && mpc::read_container_index(index, index_bytes, x) ? static_cast<int>(x.version) : 0;
    } catch (...) {
        return 0;
    }
}

mpc_status mpc_index_aux(const uint8_t* index, size_t index_bytes, int stream, uint64_t* out, uint16_t* prev, uint8_t* state, uint16_t* dc,
                         size_t capacity, size_t* n_entries) {
    return guarded([&]() -> mpc_status {
        if (!index || !n_entries) return fail(MPC_ERR_ARGUMENT, "null argument");
        mpc::ContainerIndex x;
        if (!mpc::read_container_index(index, index_bytes, x)) return fail(MPC_ERR_BITSTREAM, "not a seek index");
        if (stream < 0 || stream >= static_cast<int>(x.streams.size())) return fail(MPC_ERR_ARGUMENT, "stream index %d out of range", stream);
        const std::vector<mpc::IndexAux>& aux = x.streams[static_cast<size_t>(stream)].aux;
        *n_entries = aux.size();
        if (!out && !prev && !state && !dc) return MPC_OK;
        if (capacity < aux.size()) return fail(MPC_ERR_ARGUMENT, "capacity %zu for %zu entries", capacity, aux.size());
        for (size_t k = 0; k < aux.size(); ++k) {
            if (out) out[k] = aux[k].out;
            if (prev) prev[k] = aux[k].prev;
            if (state) state[k] = aux[k].state;
            if (dc) dc[k] = aux[k].dc;
        }
        return MPC_OK;
    });
}

mpc_status mpc_window_chunks_by_index(const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes, const mpc_rect* rect,
                                      unsigned flags, uint64_t* chunks, int* route) {
    return guarded([&]() -> mpc_status {
        if (!bytes || !index || !rect || !chunks || !route) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (flags & ~MPC_REGION_PARSE_ALL) return fail(MPC_ERR_ARGUMENT, "flags 0x%x", flags);
        std::vector<uint64_t> got;
        const int verdict = mpc::window_chunks_by_index(bytes, nbytes, index, index_bytes, rect->x, rect->y, rect->width, rect->height,
                                                        (flags & MPC_REGION_PARSE_ALL) != 0, got, route);
        if (verdict == 1) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
        if (verdict == 2) return fail(MPC_ERR_ARGUMENT, "rectangle %dx%d at (%d, %d) is empty or not inside the frame", rect->width, rect->height, rect->x, rect->y);
        std::memcpy(chunks, got.data(), sizeof(uint64_t) * got.size());
        return MPC_OK;
    });
}

mpc_status mpc_index_info(const uint8_t* index, size_t index_bytes, mpc_index_header* info) {
    return guarded([&]() -> mpc_status {
        if (!index || !info) return fail(MPC_ERR_ARGUMENT, "null argument");
        mpc::ContainerIndex x;
        if (!mpc::read_container_index(index, index_bytes, x)) return fail(MPC_ERR_BITSTREAM, "not a seek index");
        info->interval = static_cast<int>(x.interval);
        info->n_streams = static_cast<int>(x.streams.size());
        info->serial_only = x.serial_only ? 1 : 0;
        info->width = x.width;
        info->height = x.height;
        info->K = x.K;
        info->block_size = x.block_size;
        info->container_bytes = x.nbytes;
        return MPC_OK;
    });
}

mpc_status mpc_index_stream(const uint8_t* index, size_t index_bytes, int stream, mpc_index_stream_info* info, uint64_t* checkpoints,
                            size_t capacity) {
    return guarded([&]() -> mpc_status {
        if (!index || !info) return fail(MPC_ERR_ARGUMENT, "null argument");
        mpc::ContainerIndex x;
        if (!mpc::read_container_index(index, index_bytes, x)) return fail(MPC_ERR_BITSTREAM, "not a seek index");
        if (stream < 0 || stream >= static_cast<int>(x.streams.size())) return fail(MPC_ERR_ARGUMENT, "stream index %d out of range", stream);
        const mpc::IndexStream& s = x.streams[static_cast<size_t>(stream)];
        info->mode = static_cast<int>(s.mode);
        info->packed = static_cast<int>(s.packed);
        info->m = s.m;
        info->n_coded = s.n_coded;
        info->expect = s.expect;
        info->wrapper_bit = s.wrapper_bit;
        info->end_bit = s.end_bit;
        info->n_checkpoints = s.checkpoints.size();
        if (checkpoints) {
            if (capacity < s.checkpoints.size()) return fail(MPC_ERR_ARGUMENT, "capacity %zu for %zu checkpoints", capacity, s.checkpoints.size());
            if (!s.checkpoints.empty()) std::memcpy(checkpoints, s.checkpoints.data(), 8 * s.checkpoints.size());
        }
        return MPC_OK;
    });
}

mpc_status mpc_parse_container_by_index(const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes, uint16_t** symbols,
                                        size_t* n_symbols, int* route) {
    return guarded([&]() -> mpc_status {
        if (!bytes || !index || !symbols || !n_symbols || !route) return fail(MPC_ERR_ARGUMENT, "null argument");
        mpc::CodedStreams s;
        if (!mpc::read_compressed_coded_by_index(bytes, nbytes, index, index_bytes, s, route)) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
        size_t total = s.lengths.size();
        for (const std::vector<uint16_t>& v : s.codes) total += v.size();
        uint16_t* out = static_cast<uint16_t*>(std::malloc(total ? 2 * total : 2));
        if (!out) return fail(MPC_ERR_ALLOC, "out of memory");
        size_t at = 0;
        auto add = [&](const std::vector<uint16_t>& v) {
            if (!v.empty()) std::memcpy(out + at, v.data(), 2 * v.size());
            at += v.size();
        };
        add(s.lengths);
        for (const std::vector<uint16_t>& v : s.codes) add(v);
        *symbols = out;
        *n_symbols = total;
        return MPC_OK;
    });
}

mpc_status mpc_parse_container_window_by_index(const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes,
                                               const mpc_rect* rect, unsigned flags, uint16_t** symbols, size_t* n_symbols,
                                               uint64_t* ranges, int* route) {
    return guarded([&]() -> mpc_status {
        if (!bytes || !index || !rect || !symbols || !n_symbols || !ranges || !route) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (flags & ~MPC_REGION_PARSE_ALL) return fail(MPC_ERR_ARGUMENT, "flags 0x%x", flags);
        std::vector<uint16_t> got;
        std::vector<uint64_t> r;
        const int verdict = mpc::read_window_by_index(bytes, nbytes, index, index_bytes, rect->x, rect->y, rect->width, rect->height,
                                                      (flags & MPC_REGION_PARSE_ALL) != 0, got, r, route);
        if (verdict == 1) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
        if (verdict == 2) return fail(MPC_ERR_ARGUMENT, "rectangle %dx%d at (%d, %d) is empty or not inside the frame", rect->width, rect->height, rect->x, rect->y);
        uint16_t* out = static_cast<uint16_t*>(std::malloc(got.empty() ? 2 : 2 * got.size()));
        if (!out) return fail(MPC_ERR_ALLOC, "out of memory");
        if (!got.empty()) std::memcpy(out, got.data(), 2 * got.size());
        std::memcpy(ranges, r.data(), sizeof(uint64_t) * r.size());
        *symbols = out;
        *n_symbols = got.size();
        return MPC_OK;
    });
}

mpc_status mpc_truncate_container(const uint8_t* bytes, size_t nbytes, int steps, uint8_t** out, size_t* out_bytes) {
    return guarded([&]() -> mpc_status {
        if (!bytes || !out || !out_bytes) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (steps < 1) return fail(MPC_ERR_ARGUMENT, "steps must be at least 1");
        std::vector<uint8_t> cut;
        if (!mpc::truncate_container(bytes, nbytes, steps, cut)) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
        uint8_t* copy = static_cast<uint8_t*>(std::malloc(cut.empty() ? 1 : cut.size()));
        if (!copy) return fail(MPC_ERR_ALLOC, "out of memory");
        if (!cut.empty()) std::memcpy(copy, cut.data(), cut.size());
        *out = copy;
        *out_bytes = cut.size();
        return MPC_OK;
    });
}

mpc_status mpc_transcode_container(const uint8_t* bytes, size_t nbytes, const mpc_view* view, uint8_t** out, size_t* out_bytes) {
    return guarded([&]() -> mpc_status {
        if (!bytes || !view || !out || !out_bytes) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (const char* why = transcode_argument_error(*view)) return fail(MPC_ERR_ARGUMENT, "%s", why);
        int width, height, K, block_size;
        if (!mpc::container_info(bytes, nbytes, &width, &height, &K, &block_size)) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
        const mpc_rect rect = view_rect(*view, width, height);
        const std::string why = mpc::transcode_rect_error(width, height, block_size, rect.x, rect.y, rect.width, rect.height);
        if (!why.empty()) return fail(MPC_ERR_ARGUMENT, "%s", why.c_str());
        std::vector<uint8_t> made;
        const int verdict = mpc::transcode_container(bytes, nbytes, rect.x, rect.y, rect.width, rect.height, view->steps, made);
        if (verdict == 1) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
        if (verdict == 2) return fail(MPC_ERR_BITSTREAM, "Invalid bitstream");
        if (verdict != 0) return fail(MPC_ERR_ARGUMENT, "rectangle %dx%d at (%d, %d) is empty or not inside the frame", rect.width, rect.height, rect.x, rect.y);
        uint8_t* copy = static_cast<uint8_t*>(std::malloc(made.empty() ? 1 : made.size()));
        if (!copy) return fail(MPC_ERR_ALLOC, "out of memory");
        if (!made.empty()) std::memcpy(copy, made.data(), made.size());
        *out = copy;
        *out_bytes = made.size();
        return MPC_OK;
    });
}

mpc_status mpc_compose_container(const uint8_t* const* bytes, const size_t* nbytes, int n_sources, const mpc_part* parts, int n_parts,
                                 int width, int height, uint8_t** out, size_t* out_bytes) {
    return guarded([&]() -> mpc_status {
        if (!bytes || !nbytes || !parts || !out || !out_bytes) return fail(MPC_ERR_ARGUMENT, "null argument");
        const std::vector<mpc::ComposePart> pieces = compose_parts(parts, n_parts);
        std::vector<uint8_t> made;
        std::string why;
        const int verdict = mpc::compose_container(bytes, nbytes, n_sources, pieces.data(), n_parts, width, height, made, why);
        if (verdict != 0) return fail(verdict == 1 ? MPC_ERR_BITSTREAM : MPC_ERR_ARGUMENT, "%s", why.c_str());
        return give_blob(made, out, out_bytes);
    });
}

mpc_status mpc_parse_container_view_by_index(const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes,
                                             const mpc_view* view, unsigned flags, uint16_t** symbols, size_t* n_symbols, uint64_t* ranges,
                                             int* route) {
    return guarded([&]() -> mpc_status {
        if (!bytes || !index || !view || !symbols || !n_symbols || !ranges || !route) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (flags & ~MPC_VIEW_PARSE_ALL) return fail(MPC_ERR_ARGUMENT, "flags 0x%x", flags);
        if (const char* why = view_argument_error(*view)) return fail(MPC_ERR_ARGUMENT, "%s", why);
        int width, height, K, block_size;
        if (!mpc::container_info(bytes, nbytes, &width, &height, &K, &block_size)) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
        const mpc_rect rect = view_rect(*view, width, height);
        std::vector<uint16_t> got;
        std::vector<uint64_t> r;
        const int verdict = mpc::read_window_by_index(bytes, nbytes, index, index_bytes, rect.x, rect.y, rect.width, rect.height,
                                                      (flags & MPC_VIEW_PARSE_ALL) != 0, got, r, route, view->steps);
        if (verdict == 1) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
        if (verdict == 2) return fail(MPC_ERR_ARGUMENT, "rectangle %dx%d at (%d, %d) is empty or not inside the frame", rect.width, rect.height, rect.x, rect.y);
        uint16_t* out = static_cast<uint16_t*>(std::malloc(got.empty() ? 2 : 2 * got.size()));
        if (!out) return fail(MPC_ERR_ALLOC, "out of memory");
        if (!got.empty()) std::memcpy(out, got.data(), 2 * got.size());
        std::memcpy(ranges, r.data(), sizeof(uint64_t) * r.size());
        *symbols = out;
        *n_symbols = got.size();
        return MPC_OK;
    });
}

}  // extern "C"
