// mpcodec_patch.cpp -- product: the delta stream's patches (include/mpcodec.h, "patch"; DESIGN.md 4, "Delta stream"): the host-only
// entry points of the format (host_patch.h) and the receiver, a session that keeps the current frame in device memory and writes only
// a patch's listed tiles into it: the unchanged mpc_decode_image_device decodes the patch's container -- the packed frame of the
// listed tiles, an ordinary frame -- into staging, and mp_tile_unpack_kernel (mp_delta.hip) puts its tiles in their places.  A
// version-2 patch carries the container's seek index: its container goes through mpc_decode_images_indexed_device instead, which
// parses the entropy codes on the device.
#include <cstring>
#include <string>

#include "host_delta.h"
#include "host_patch.h"
#include "mpc_internal.h"

struct mpc_patch_decoder {
    mpc_context* ctx = nullptr;
    int width = 0, height = 0;
    long long tiles = 0;
    GrowBuffer kept{GrowBuffer::kDevice};       // the current frame, tight; sized once
    GrowBuffer staging{GrowBuffer::kDevice};    // grow-only: a patch's decoded pixels (the packed frame, or a key patch's whole frame)
    GrowBuffer list{GrowBuffer::kDevice};       // grow-only: the unpack kernel's error word, then the list
    hipStream_t stream = nullptr;
    bool has_key = false;                       // a key patch has been applied (and no apply has failed half-way since)
    uint32_t expected = 0;                      // the sequence the next non-key patch must carry
    bool changed_all = false;                   // the last apply's list is every tile
    std::vector<int32_t> changed;               // else this
    int route = -1;                             // the last apply's decode: 0 parsed on the device, 1 serial, -1 none (an empty patch)
    ~mpc_patch_decoder() {
        if (stream) {
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
    }
};

namespace {

void report(const mpc::PatchInfo& p, struct mpc_patch_info* info) {
    info->width = p.width;
    info->height = p.height;
    info->sequence = p.sequence;
    info->key = p.key ? 1 : 0;
    info->n = static_cast<int>(p.n);
    info->tiles = static_cast<int>(p.tiles);
    info->container_offset = p.container_offset;
    info->container_bytes = p.container_bytes;
}

mpc_status give(const std::vector<uint8_t>& blob, uint8_t** bytes, size_t* nbytes) {
    uint8_t* out = static_cast<uint8_t*>(std::malloc(blob.size()));
    if (!out) return fail(MPC_ERR_ALLOC, "no patch");
    std::memcpy(out, blob.data(), blob.size());
    *bytes = out;
    *nbytes = blob.size();
    return MPC_OK;
}

}  // namespace

extern "C" {

mpc_status mpc_patch_make(int width, int height, uint32_t sequence, int key, const int32_t* tiles, int n, const uint8_t* container,
                          size_t container_bytes, uint8_t** bytes, size_t* nbytes) {
    return guarded([&]() -> mpc_status {
        if (!bytes || !nbytes) return fail(MPC_ERR_ARGUMENT, "null argument");
        const std::string why = mpc::patch_make_error(width, height, key != 0, tiles, n, container, container_bytes);
        if (!why.empty()) return fail(MPC_ERR_ARGUMENT, "%s", why.c_str());
        return give(mpc::patch_make(width, height, sequence, key != 0, tiles, n, container, container_bytes), bytes, nbytes);
    });
}

mpc_status mpc_patch_make_indexed(int width, int height, uint32_t sequence, int key, const int32_t* tiles, int n, const uint8_t* container,
                                  size_t container_bytes, const uint8_t* index, size_t index_bytes, uint8_t** bytes, size_t* nbytes) {
    return guarded([&]() -> mpc_status {
        if (!bytes || !nbytes) return fail(MPC_ERR_ARGUMENT, "null argument");
        const std::string why = mpc::patch_make_error(width, height, key != 0, tiles, n, container, container_bytes, index, index_bytes);
        if (!why.empty()) return fail(MPC_ERR_ARGUMENT, "%s", why.c_str());
        return give(mpc::patch_make(width, height, sequence, key != 0, tiles, n, container, container_bytes, index, index_bytes), bytes, nbytes);
    });
}

mpc_status mpc_patch_index(const uint8_t* bytes, size_t nbytes, size_t* index_offset, size_t* index_bytes) {
    return guarded([&]() -> mpc_status {
        if (!bytes || !index_offset || !index_bytes) return fail(MPC_ERR_ARGUMENT, "null argument");
        mpc::PatchInfo p;
        const std::string why = mpc::patch_parse(bytes, nbytes, &p, nullptr);
        if (!why.empty()) return fail(MPC_ERR_BITSTREAM, "Invalid patch: %s", why.c_str());
        *index_offset = p.index_offset;
        *index_bytes = p.index_bytes;
        return MPC_OK;
    });
}

mpc_status mpc_patch_add_index(const uint8_t* patch, size_t nbytes, int interval, size_t index_min_bytes, uint8_t** out, size_t* out_bytes) {
    return guarded([&]() -> mpc_status {
        if (!patch || !out || !out_bytes) return fail(MPC_ERR_ARGUMENT, "null argument");
        unsigned every = 0;
        if (const mpc_status bad = index_interval_of(interval, &every)) return bad;
        mpc::PatchInfo p;
        const std::string why = mpc::patch_parse(patch, nbytes, &p, nullptr);
        if (!why.empty()) return fail(MPC_ERR_BITSTREAM, "Invalid patch: %s", why.c_str());
        return give(mpc::patch_add_index(patch, p, every, index_min_bytes), out, out_bytes);
    });
}

mpc_status mpc_patch_strip_index(const uint8_t* patch, size_t nbytes, uint8_t** out, size_t* out_bytes) {
    return guarded([&]() -> mpc_status {
        if (!patch || !out || !out_bytes) return fail(MPC_ERR_ARGUMENT, "null argument");
        mpc::PatchInfo p;
        const std::string why = mpc::patch_parse(patch, nbytes, &p, nullptr);
        if (!why.empty()) return fail(MPC_ERR_BITSTREAM, "Invalid patch: %s", why.c_str());
        return give(mpc::patch_strip_index(patch, p), out, out_bytes);
    });
}

mpc_status mpc_patch_info(const uint8_t* bytes, size_t nbytes, struct mpc_patch_info* info) {
    return guarded([&]() -> mpc_status {
        if (!bytes || !info) return fail(MPC_ERR_ARGUMENT, "null argument");
        mpc::PatchInfo p;
        const std::string why = mpc::patch_parse(bytes, nbytes, &p, nullptr);
        if (!why.empty()) return fail(MPC_ERR_BITSTREAM, "Invalid patch: %s", why.c_str());
        report(p, info);
        return MPC_OK;
    });
}

mpc_status mpc_patch_tiles(const uint8_t* bytes, size_t nbytes, int32_t* tiles, int capacity, int* n) {
    return guarded([&]() -> mpc_status {
        if (!bytes || !n || (capacity > 0 && !tiles)) return fail(MPC_ERR_ARGUMENT, "null argument");
        mpc::PatchInfo p;
        std::vector<int32_t> list;
        const std::string why = mpc::patch_parse(bytes, nbytes, &p, &list);
        if (!why.empty()) return fail(MPC_ERR_BITSTREAM, "Invalid patch: %s", why.c_str());
        *n = static_cast<int>(p.n);
        if (capacity < p.n) return capacity > 0 ? fail(MPC_ERR_ARGUMENT, "room for %d tiles, %lld listed", capacity, p.n) : MPC_OK;
        for (long long t = 0; t < p.n; ++t) tiles[t] = p.key ? static_cast<int32_t>(t) : list[static_cast<size_t>(t)];
        return MPC_OK;
    });
}

mpc_status mpc_patch_decoder_create(mpc_context* c, int width, int height, mpc_patch_decoder** out) {
    return guarded([&]() -> mpc_status {
        if (!c || !out) return fail(MPC_ERR_ARGUMENT, "null argument");
        *out = nullptr;
        const long long tiles = mpc::patch_frame_tiles(width, height);
        if (tiles == 0) return fail(MPC_ERR_ARGUMENT, "bad geometry");
        if (c->device < 0) return no_device();
        std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
        HIP_TRY(hipSetDevice(c->device));
        std::unique_ptr<mpc_patch_decoder> p(new mpc_patch_decoder);
        p->ctx = c;
        p->width = width;
        p->height = height;
        p->tiles = tiles;
        const size_t frame_bytes = 3 * static_cast<size_t>(width) * static_cast<size_t>(height);
        if (const mpc_status gs = p->kept.reserve(frame_bytes, "patch decoder frame"); gs != MPC_OK) return gs;
        if (const mpc_status gs = p->list.reserve(256 + sizeof(int32_t), "patch decoder list"); gs != MPC_OK) return gs;
        HIP_TRY(hipMemset(p->kept.data(), 0, frame_bytes));                 // black until the first key patch
        HIP_TRY(hipMemset(p->list.data(), 0, sizeof(int)));
        HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
        *out = p.release();
        return MPC_OK;
    });
}

void mpc_patch_decoder_destroy(mpc_patch_decoder* p) {
    if (!p) return;
    if (p->ctx && p->ctx->device >= 0) (void)hipSetDevice(p->ctx->device);
    delete p;
}

mpc_status mpc_patch_apply(mpc_patch_decoder* p, const uint8_t* patch, size_t nbytes, struct mpc_patch_info* info) {
    return guarded([&]() -> mpc_status {
        if (!p || !patch || !info) return fail(MPC_ERR_ARGUMENT, "null argument");
        mpc_context* c = p->ctx;
        if (c->device < 0) return no_device();
        // every check first: nothing reaches the kept frame, the list or the expected sequence before all of them have passed
        mpc::PatchInfo pi;
        std::vector<int32_t> listed;
        const std::string why = mpc::patch_parse(patch, nbytes, &pi, &listed);
        if (!why.empty()) return fail(MPC_ERR_BITSTREAM, "Invalid patch: %s", why.c_str());
        if (pi.width != p->width || pi.height != p->height)
            return fail(MPC_ERR_ARGUMENT, "a patch of %d x %d frames for a session of %d x %d", pi.width, pi.height, p->width, p->height);
        if (!pi.key) {
            if (!p->has_key) return fail(MPC_ERR_ARGUMENT, "patch %u is no key patch and the session has had none", pi.sequence);
            if (pi.sequence != p->expected) return fail(MPC_ERR_ARGUMENT, "patch %u where patch %u is expected", pi.sequence, p->expected);
        }
        std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
        HIP_TRY(hipSetDevice(c->device));
        hipStream_t s = p->stream;
        int route = -1;
        if (pi.n > 0) {
            const uint8_t* container = patch + pi.container_offset;
            int cw = 0, ch = 0, cK = 0, cbs = 0;
            if (!mpc::container_info(container, pi.container_bytes, &cw, &ch, &cK, &cbs)) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
            if (cbs != c->block_size || cK != c->K)
                return fail(MPC_ERR_ARGUMENT, "a container of block size %d and K %d for a context of %d and %d", cbs, cK, c->block_size, c->K);
            const mpc::PackGeometry g = mpc::pack_geometry(pi.n, MPC_DELTA_PACK_ROWS);
            const int want_w = pi.key ? p->width : 8 * g.cols, want_h = pi.key ? p->height : 8 * g.rows;
            if (cw != want_w || ch != want_h) return fail(MPC_ERR_BITSTREAM, "Invalid patch: a container of %d x %d where %d x %d is due", cw, ch, want_w, want_h);
            const size_t pixels = 3 * static_cast<size_t>(want_w) * static_cast<size_t>(want_h);
            if (const mpc_status gs = p->staging.reserve(pixels, "patch decoder staging"); gs != MPC_OK) return gs;
            if (!pi.key)
                if (const mpc_status gs = p->list.reserve(256 + sizeof(int32_t) * listed.size(), "patch decoder list"); gs != MPC_OK) return gs;
            uint8_t* staged = reinterpret_cast<uint8_t*>(p->staging.data());
            int w = 0, h = 0;
            // the decoder's own refusals, status and text: it returns when the pixels are complete and its error words are read.  A
            // version-2 patch: the indexed route of the same decoder, the index section read where it lies (its readers go bytewise);
            // an index the decoder refuses costs the serial route it falls back to, never the patch
            route = 1;
            const uint8_t* index = pi.index_bytes ? patch + pi.index_offset : nullptr;
            if (const mpc_status ds = index ? mpc_decode_images_indexed_device(c, &container, &pi.container_bytes, &index, &pi.index_bytes, 1, &staged,
                                                                               &pixels, &w, &h, &route)
                                            : mpc_decode_image_device(c, container, pi.container_bytes, staged, pixels, &w, &h);
                ds != MPC_OK)
                return ds;
            if (w != want_w || h != want_h) return fail(MPC_ERR_BITSTREAM, "Invalid patch: decoded %d x %d where %d x %d is due", w, h, want_w, want_h);
            // from here on the kept frame is written: only the device itself can still fail, and then the session wants a key patch
            struct Broken {
                mpc_patch_decoder* p;
                bool keep = false;
                ~Broken() {
                    if (!keep) p->has_key = false;
                }
            } broken{p};
            uint8_t* kept = reinterpret_cast<uint8_t*>(p->kept.data());
            if (pi.key) {
                HIP_TRY(hipMemcpyAsync(kept, staged, pixels, hipMemcpyDeviceToDevice, s));
                HIP_TRY(hipStreamSynchronize(s));
            } else {
                int* d_error = reinterpret_cast<int*>(p->list.data());
                int32_t* d_list = reinterpret_cast<int32_t*>(p->list.data() + 256);
                HIP_TRY(hipMemsetAsync(d_error, 0, sizeof(int), s));
                HIP_TRY(hipMemcpyAsync(d_list, listed.data(), sizeof(int32_t) * listed.size(), hipMemcpyHostToDevice, s));
                if (const int e = mpc::launch_tile_unpack(staged, g.stride, d_list, pi.n, g.rows, g.cols, kept, p->width, p->height,
                                                          3 * static_cast<size_t>(p->width), d_error, s);
                    e != 0) {
                    (void)hipStreamSynchronize(s);                          // `listed` is still on its way
                    return launch_failed(e);
                }
                int flagged = 0;
                HIP_TRY(hipMemcpyAsync(&flagged, d_error, sizeof(int), hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                if (flagged) return fail(MPC_ERR_HIP, "the unpack kernel met a tile outside the frame that the host's check had passed");
            }
            broken.keep = true;
        }
        if (pi.key) p->has_key = true;
        p->expected = pi.sequence + 1;
        p->changed_all = pi.key;
        p->changed.swap(listed);
        p->route = route;
        report(pi, info);
        return MPC_OK;
    });
}

mpc_status mpc_patch_frame_device(mpc_patch_decoder* p, uint8_t** d_rgb) {
    if (!p || !d_rgb) return fail(MPC_ERR_ARGUMENT, "null argument");
    *d_rgb = reinterpret_cast<uint8_t*>(p->kept.data());
    return MPC_OK;
}

mpc_status mpc_patch_read(mpc_patch_decoder* p, uint8_t* rgb, size_t row_stride) {
    return guarded([&]() -> mpc_status {
        if (!p || !rgb) return fail(MPC_ERR_ARGUMENT, "null argument");
        const size_t row = 3 * static_cast<size_t>(p->width);
        if (row_stride != 0 && row_stride < row) return fail(MPC_ERR_ARGUMENT, "row_stride %zu for %d pixels", row_stride, p->width);
        HIP_TRY(hipSetDevice(p->ctx->device));
        HIP_TRY(hipMemcpy2DAsync(rgb, row_stride ? row_stride : row, p->kept.data(), row, row, static_cast<size_t>(p->height), hipMemcpyDeviceToHost,
                                 p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        return MPC_OK;
    });
}

int mpc_patch_last_route(const mpc_patch_decoder* p) { return p ? p->route : -1; }

mpc_status mpc_patch_changed(const mpc_patch_decoder* p, int32_t* tiles, int capacity, int* n) {
    if (!p || !n || (capacity > 0 && !tiles)) return fail(MPC_ERR_ARGUMENT, "null argument");
    const long long count = p->changed_all ? p->tiles : static_cast<long long>(p->changed.size());
    *n = static_cast<int>(count);
    if (capacity < count) return capacity > 0 ? fail(MPC_ERR_ARGUMENT, "room for %d tiles, %lld changed", capacity, count) : MPC_OK;
    for (long long t = 0; t < count; ++t) tiles[t] = p->changed_all ? static_cast<int32_t>(t) : p->changed[static_cast<size_t>(t)];
    return MPC_OK;
}

}  // extern "C"
