// mpcodec_delta.cpp -- product: the delta encoder (include/mpcodec.h, "delta"; DESIGN.md 4, "Encoder: changed tiles only").
// A session keeps the last frame and its records in device memory; a call finds the changed tiles on the device (mp_delta.hip),
// pursues only those through the unchanged tile encoder, and makes the container from the whole frame's records as a compose does --
// or, as the sender of a delta stream (mpc_delta_encode_patch[_indexed]; include/mpcodec.h, "patch"), a patch: the list and the
// container of the packed frame of the listed tiles alone, with the container's seek index where one is asked for.
#include <cstring>
#include <string>

#include "host_delta.h"
#include "host_patch.h"
#include "mpc_delta_session.h"

static_assert(mpc::kDeltaPackRows == MPC_DELTA_PACK_ROWS, "one value for the packed frame's tile rows");

extern "C" {

mpc_status mpc_changed_tiles(const uint8_t* prev, size_t prev_stride, const uint8_t* cur, size_t cur_stride, int width, int height,
                             int block_size, int32_t* tiles, int* n) {
    return guarded([&]() -> mpc_status {
        if (!prev || !cur || !tiles || !n) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (width < 1 || height < 1 || block_size < 1 || block_size > 8) return fail(MPC_ERR_ARGUMENT, "bad geometry");
        const size_t row = 3 * static_cast<size_t>(width);
        if ((prev_stride != 0 && prev_stride < row) || (cur_stride != 0 && cur_stride < row))
            return fail(MPC_ERR_ARGUMENT, "a row stride below %zu for %d pixels", row, width);
        const long long all = ((static_cast<long long>(width) + block_size - 1) / block_size) * ((static_cast<long long>(height) + block_size - 1) / block_size);
        if (all >= (1LL << 31)) return fail(MPC_ERR_ARGUMENT, "bad geometry");
        *n = static_cast<int>(mpc::changed_tiles(prev, prev_stride ? prev_stride : row, cur, cur_stride ? cur_stride : row, width, height, block_size, tiles));
        return MPC_OK;
    });
}

mpc_status mpc_delta_pack_geometry(long long n, int rows, int* packed_rows, int* packed_cols, size_t* packed_stride, size_t* packed_bytes) {
    if (!packed_rows || !packed_cols || !packed_stride || !packed_bytes) return fail(MPC_ERR_ARGUMENT, "null argument");
    if (n < 0 || rows < 1 || n >= (1LL << 31)) return fail(MPC_ERR_ARGUMENT, "n %lld, rows %d", n, rows);
    const mpc::PackGeometry g = mpc::pack_geometry(n, rows);
    *packed_rows = g.rows;
    *packed_cols = g.cols;
    *packed_stride = g.stride;
    *packed_bytes = g.bytes;
    return MPC_OK;
}

mpc_status mpc_tile_diff_device(mpc_context* c, uint8_t* d_kept, const uint8_t* d_rgb, int width, int height, size_t row_stride,
                                int32_t* d_list, int32_t* d_count, void* stream) {
    return guarded([&]() -> mpc_status {
        if (!c || !d_kept || !d_rgb || !d_list || !d_count) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (c->device < 0) return no_device();
        if (width < 1 || height < 1) return fail(MPC_ERR_ARGUMENT, "bad geometry");
        const size_t row = 3 * static_cast<size_t>(width), stride = row_stride ? row_stride : row;
        if (stride < row) return fail(MPC_ERR_ARGUMENT, "row_stride %zu for %d pixels", row_stride, width);
        const long long tiles = ((static_cast<long long>(width) + 7) / 8) * ((static_cast<long long>(height) + 7) / 8);
        if (tiles >= (1LL << 31)) return fail(MPC_ERR_ARGUMENT, "bad geometry");
        std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
        HIP_TRY(hipSetDevice(c->device));
        if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
        if (const mpc_status gs = c->delta_scratch.reserve(mpc::tile_diff_scratch_bytes(tiles), "diff scratch"); gs != MPC_OK) return gs;
        const int err = mpc::launch_tile_diff(d_kept, d_rgb, width, height, stride, d_list, d_count, c->delta_scratch.data(), stream);
        if (err != 0) return launch_failed(err);
        return MPC_OK;
    });
}

mpc_status mpc_changed_tiles_tolerance(const uint8_t* prev, size_t prev_stride, const uint8_t* cur, size_t cur_stride, int width, int height,
                                       int block_size, uint32_t tolerance, int32_t* tiles, int* n, uint32_t* sse) {
    return guarded([&]() -> mpc_status {
        if (!prev || !cur || !tiles || !n) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (width < 1 || height < 1 || block_size < 1 || block_size > 8) return fail(MPC_ERR_ARGUMENT, "bad geometry");
        const size_t row = 3 * static_cast<size_t>(width);
        if ((prev_stride != 0 && prev_stride < row) || (cur_stride != 0 && cur_stride < row))
            return fail(MPC_ERR_ARGUMENT, "a row stride below %zu for %d pixels", row, width);
        const long long all = ((static_cast<long long>(width) + block_size - 1) / block_size) * ((static_cast<long long>(height) + block_size - 1) / block_size);
        if (all >= (1LL << 31)) return fail(MPC_ERR_ARGUMENT, "bad geometry");
        *n = static_cast<int>(mpc::changed_tiles_tolerance(prev, prev_stride ? prev_stride : row, cur, cur_stride ? cur_stride : row, width, height,
                                                           block_size, tolerance, tiles, sse));
        return MPC_OK;
    });
}

mpc_status mpc_tile_diff_tolerance_device(mpc_context* c, uint8_t* d_kept, const uint8_t* d_rgb, int width, int height, size_t row_stride,
                                          uint32_t tolerance, int32_t* d_list, int32_t* d_count, uint32_t* d_sse, void* stream) {
    return guarded([&]() -> mpc_status {
        if (!c || !d_kept || !d_rgb || !d_list || !d_count) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (c->device < 0) return no_device();
        if (width < 1 || height < 1) return fail(MPC_ERR_ARGUMENT, "bad geometry");
        const size_t row = 3 * static_cast<size_t>(width), stride = row_stride ? row_stride : row;
        if (stride < row) return fail(MPC_ERR_ARGUMENT, "row_stride %zu for %d pixels", row_stride, width);
        const long long tiles = ((static_cast<long long>(width) + 7) / 8) * ((static_cast<long long>(height) + 7) / 8);
        if (tiles >= (1LL << 31)) return fail(MPC_ERR_ARGUMENT, "bad geometry");
        std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
        HIP_TRY(hipSetDevice(c->device));
        if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
        if (const mpc_status gs = c->delta_scratch.reserve(mpc::tile_diff_scratch_bytes(tiles), "diff scratch"); gs != MPC_OK) return gs;
        const int err = mpc::launch_tile_diff_tolerance(d_kept, d_rgb, width, height, stride, tolerance, d_list, d_count, d_sse, nullptr,
                                                        c->delta_scratch.data(), stream);
        if (err != 0) return launch_failed(err);
        return MPC_OK;
    });
}

mpc_status mpc_pack_tiles_device(mpc_context* c, const uint8_t* d_rgb, int width, int height, size_t row_stride, const int32_t* d_list, int n,
                                 int rows, uint8_t* d_packed, size_t packed_stride, void* stream) {
    return guarded([&]() -> mpc_status {
        if (!c || !d_rgb || !d_list || !d_packed) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (c->device < 0) return no_device();
        if (width < 1 || height < 1 || n < 1 || rows < 1) return fail(MPC_ERR_ARGUMENT, "bad geometry");
        const size_t row = 3 * static_cast<size_t>(width), stride = row_stride ? row_stride : row;
        if (stride < row) return fail(MPC_ERR_ARGUMENT, "row_stride %zu for %d pixels", row_stride, width);
        const mpc::PackGeometry g = mpc::pack_geometry(n, rows);
        const size_t to = packed_stride ? packed_stride : g.stride;
        if (to < g.stride || to % 8 != 0 || reinterpret_cast<uintptr_t>(d_packed) % 8 != 0)
            return fail(MPC_ERR_ARGUMENT, "the packed frame: an 8-byte aligned base and a stride that is a multiple of 8 and at least %zu", g.stride);
        HIP_TRY(hipSetDevice(c->device));
        if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
        const int err = mpc::launch_tile_pack(d_rgb, width, height, stride, d_list, n, g.rows, g.cols, d_packed, to, stream);
        if (err != 0) return launch_failed(err);
        return MPC_OK;
    });
}

mpc_status mpc_unpack_tiles_device(mpc_context* c, const uint8_t* d_packed, size_t packed_stride, const int32_t* d_list, int n, int rows,
                                   uint8_t* d_rgb, int width, int height, size_t row_stride, void* stream) {
    return guarded([&]() -> mpc_status {
        if (!c || !d_packed || !d_list || !d_rgb) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (c->device < 0) return no_device();
        if (width < 1 || height < 1 || n < 1 || rows < 1) return fail(MPC_ERR_ARGUMENT, "bad geometry");
        const size_t row = 3 * static_cast<size_t>(width), stride = row_stride ? row_stride : row;
        if (stride < row) return fail(MPC_ERR_ARGUMENT, "row_stride %zu for %d pixels", row_stride, width);
        if (mpc::patch_frame_tiles(width, height) == 0) return fail(MPC_ERR_ARGUMENT, "bad geometry");
        const mpc::PackGeometry g = mpc::pack_geometry(n, rows);
        const size_t from = packed_stride ? packed_stride : g.stride;
        if (from < g.stride || from % 8 != 0 || reinterpret_cast<uintptr_t>(d_packed) % 8 != 0)
            return fail(MPC_ERR_ARGUMENT, "the packed frame: an 8-byte aligned base and a stride that is a multiple of 8 and at least %zu", g.stride);
        HIP_TRY(hipSetDevice(c->device));
        if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
        if (const mpc_status fs = crop_flag(c); fs != MPC_OK) return fs;
        const int err = mpc::launch_tile_unpack(d_packed, from, d_list, n, g.rows, g.cols, d_rgb, width, height, stride, c->d_crop_flag, stream);
        if (err != 0) return launch_failed(err);
        return MPC_OK;
    });
}

mpc_status mpc_scatter_records_device(mpc_context* c, const uint16_t* d_packed_counts, const mpc_basis_choice* d_packed_choices,
                                      const int32_t* d_list, int n, uint16_t* d_counts, mpc_basis_choice* d_choices, int tiles, void* stream) {
    return guarded([&]() -> mpc_status {
        if (!c || !d_packed_counts || !d_packed_choices || !d_list || !d_counts || !d_choices) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (c->device < 0) return no_device();
        if (n < 1 || tiles < 1) return fail(MPC_ERR_ARGUMENT, "n %d, tiles %d", n, tiles);
        HIP_TRY(hipSetDevice(c->device));
        if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
        if (const mpc_status fs = crop_flag(c); fs != MPC_OK) return fs;
        const int err = mpc::launch_tile_scatter_records(d_packed_counts, reinterpret_cast<const uint32_t*>(d_packed_choices), d_list, n, c->K, d_counts,
                                                         reinterpret_cast<uint32_t*>(d_choices), tiles, c->d_crop_flag, stream);
        if (err != 0) return launch_failed(err);
        return MPC_OK;
    });
}

mpc_status mpc_delta_create(mpc_context* c, int width, int height, mpc_delta** out) {
    return guarded([&]() -> mpc_status {
        if (!c || !out) return fail(MPC_ERR_ARGUMENT, "null argument");
        *out = nullptr;
        if (width < 1 || height < 1) return fail(MPC_ERR_ARGUMENT, "bad geometry");
        if (c->device < 0) return no_device();
        const long long tiles_y = (static_cast<long long>(height) + 7) / 8, tiles = ((static_cast<long long>(width) + 7) / 8) * tiles_y;
        if (tiles >= (1LL << 31) / (3 * MPC_MAX_K)) return fail(MPC_ERR_ARGUMENT, "bad geometry");
        std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
        HIP_TRY(hipSetDevice(c->device));
        std::unique_ptr<mpc_delta> d(new mpc_delta);
        d->ctx = c;
        d->width = width;
        d->height = height;
        d->tiles_y = static_cast<int>(tiles_y);
        d->tiles = tiles;
        const size_t n_tc = 3 * static_cast<size_t>(tiles);
        const auto layout = [&](char* base) {
            Carve cv{base};
            d->d_kept = cv.take<uint8_t>(3 * static_cast<size_t>(width) * static_cast<size_t>(height));
            d->d_counts = cv.take<uint16_t>(n_tc + 2);
            d->d_choices = cv.take<mpc_basis_choice>(n_tc * static_cast<size_t>(c->K));
            d->d_list = cv.take<int32_t>(static_cast<size_t>(tiles));
            d->d_count = cv.take<int32_t>(2);
            d->d_scratch = cv.take<char>(mpc::tile_diff_scratch_bytes(tiles));
            return cv.at;
        };
        if (const mpc_status gs = d->store.reserve(layout(nullptr), "delta session"); gs != MPC_OK) return gs;
        layout(d->store.data());
        HIP_TRY(hipMemset(d->d_count, 0, 2 * sizeof(int32_t)));
        HIP_TRY(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
        *out = d.release();
        return MPC_OK;
    });
}

void mpc_delta_destroy(mpc_delta* d) {
    if (!d) return;
    if (d->ctx && d->ctx->device >= 0) (void)hipSetDevice(d->ctx->device);
    delete d;
}

mpc_status mpc_delta_changed(const mpc_delta* d, int32_t* tiles, int capacity, int* n) {
    if (!d || !n || (capacity > 0 && !tiles)) return fail(MPC_ERR_ARGUMENT, "null argument");
    const long long count = d->changed_all ? d->tiles : static_cast<long long>(d->changed.size());
    *n = static_cast<int>(count);
    if (capacity < count) return capacity > 0 ? fail(MPC_ERR_ARGUMENT, "room for %d tiles, %lld changed", capacity, count) : MPC_OK;
    for (long long t = 0; t < count; ++t) tiles[t] = d->changed_all ? static_cast<int32_t>(t) : d->changed[static_cast<size_t>(t)];
    return MPC_OK;
}

mpc_status mpc_delta_set_tolerance(mpc_delta* d, uint32_t tolerance) {
    return guarded([&]() -> mpc_status {
        if (!d) return fail(MPC_ERR_ARGUMENT, "null argument");
        std::lock_guard<std::recursive_mutex> one_host_call(d->ctx->host_calls);
        d->tolerance = tolerance;                                   // read by the next call's diff; the kept copy and the sent map stay true
        return MPC_OK;
    });
}

uint32_t mpc_delta_tolerance(const mpc_delta* d) { return d ? d->tolerance : 0u; }

mpc_status mpc_delta_held(const mpc_delta* d, int* held, uint64_t* held_sse) {
    if (!d || !held || !held_sse) return fail(MPC_ERR_ARGUMENT, "null argument");
    *held = static_cast<int>(d->held);
    *held_sse = d->held_sse;
    return MPC_OK;
}

mpc_status mpc_delta_frame_device(mpc_delta* d, uint8_t** d_rgb) {
    if (!d || !d_rgb) return fail(MPC_ERR_ARGUMENT, "null argument");
    *d_rgb = nullptr;
    if (!d->valid) return fail(MPC_ERR_ARGUMENT, "the session has no frame: no call yet, or the last one failed");
    *d_rgb = d->d_kept;
    return MPC_OK;
}

mpc_status mpc_delta_frame(mpc_delta* d, uint8_t* rgb, size_t row_stride) {
    return guarded([&]() -> mpc_status {
        if (!d || !rgb) return fail(MPC_ERR_ARGUMENT, "null argument");
        const size_t row = 3 * static_cast<size_t>(d->width);
        if (row_stride != 0 && row_stride < row) return fail(MPC_ERR_ARGUMENT, "row_stride %zu for %d pixels", row_stride, d->width);
        if (!d->valid) return fail(MPC_ERR_ARGUMENT, "the session has no frame: no call yet, or the last one failed");
        std::lock_guard<std::recursive_mutex> one_host_call(d->ctx->host_calls);
        HIP_TRY(hipSetDevice(d->ctx->device));
        // the session's calls are synchronous: nothing on its stream writes the kept copy
        HIP_TRY(hipMemcpy2DAsync(rgb, row_stride ? row_stride : row, d->d_kept, row, row, static_cast<size_t>(d->height), hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(hipStreamSynchronize(d->stream));
        return MPC_OK;
    });
}

mpc_status mpc_delta_set_emphasis(mpc_delta* d, const uint8_t* emphasis, int tiles) {
    return guarded([&]() -> mpc_status {
        if (!d) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (emphasis && tiles != d->tiles) return fail(MPC_ERR_ARGUMENT, "an emphasis map of %d tiles, the session has %lld", tiles, d->tiles);
        mpc_context* c = d->ctx;
        if (c->device < 0) return no_device();
        std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
        if (!emphasis) {
            d->has_emphasis = false;
            return MPC_OK;
        }
        HIP_TRY(hipSetDevice(c->device));
        if (const mpc_status gs = d->emphasis.reserve(static_cast<size_t>(d->tiles), "emphasis map"); gs != MPC_OK) return gs;
        // the session's calls are synchronous: nothing on its stream reads the old map
        d->has_emphasis = false;
        HIP_TRY(hipMemcpy(d->emphasis.data(), emphasis, static_cast<size_t>(d->tiles), hipMemcpyHostToDevice));
        d->has_emphasis = true;
        return MPC_OK;
    });
}

}  // extern "C"

// ---- a call in stages: mpc_delta_encode and mpc_delta_encode_patch share the first three, so the session's store advances
// identically whichever is called, and differ in what the container job of the fourth is run on (mpc_delta_session.h: the driver) ----

// 1. the frame on the device
mpc_status delta_frame(mpc_delta* d, const uint8_t* rgb, size_t row_stride, hipStream_t s, DeltaCall& call) {
    const size_t row = 3 * static_cast<size_t>(d->width);
    call.frame = rgb;
    call.stride = row_stride ? row_stride : row;
    if (!(call.flags & MPC_DELTA_DEVICE_PIXELS)) {
        if (const mpc_status gs = d->upload.reserve(row * static_cast<size_t>(d->height), "delta upload"); gs != MPC_OK) return gs;
        uint8_t* up = reinterpret_cast<uint8_t*>(d->upload.data());
        HIP_TRY(hipMemcpy2DAsync(up, row, rgb, call.stride, row, static_cast<size_t>(d->height), hipMemcpyHostToDevice, s));
        call.frame = up;
        call.stride = row;
    }
    return MPC_OK;
}

// 2., 3. the changed tiles: all of them for a key frame, else the diff's list; the kept copy becomes this frame -- with a tolerance the
// composite: this frame in the listed tiles, what it was in every other
mpc_status delta_list(mpc_delta* d, hipStream_t s, DeltaCall& call) {
    const size_t row = 3 * static_cast<size_t>(d->width);
    call.n = d->tiles;
    d->changed.clear();
    if (call.key) {
        HIP_TRY(hipMemcpy2DAsync(d->d_kept, row, call.frame, call.stride, row, static_cast<size_t>(d->height), hipMemcpyDeviceToDevice, s));
        if (call.through_pack) {
            d->changed.resize(static_cast<size_t>(call.n));
            for (long long t = 0; t < call.n; ++t) d->changed[static_cast<size_t>(t)] = static_cast<int32_t>(t);
            HIP_TRY(hipMemcpyAsync(d->d_list, d->changed.data(), sizeof(int32_t) * d->changed.size(), hipMemcpyHostToDevice, s));
            HIP_TRY(hipStreamSynchronize(s));
            d->changed.clear();
        }
        return MPC_OK;
    }
    unsigned long long held[2] = {0, 0};
    if (d->tolerance == 0) {
        if (const int e = mpc::launch_tile_diff(d->d_kept, call.frame, d->width, d->height, call.stride, d->d_list, d->d_count, d->d_scratch, s); e != 0)
            return launch_failed(e);
    } else {
        if (const mpc_status gs = d->held_totals.reserve(sizeof(held), "held totals"); gs != MPC_OK) return gs;
        unsigned long long* d_held = reinterpret_cast<unsigned long long*>(d->held_totals.data());
        if (const int e = mpc::launch_tile_diff_tolerance(d->d_kept, call.frame, d->width, d->height, call.stride, d->tolerance, d->d_list, d->d_count,
                                                          nullptr, d_held, d->d_scratch, s);
            e != 0)
            return launch_failed(e);
        HIP_TRY(hipMemcpyAsync(held, d_held, sizeof(held), hipMemcpyDeviceToHost, s));
    }
    int32_t count = -1;
    HIP_TRY(hipMemcpyAsync(&count, d->d_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (count < 0 || count > d->tiles) return fail(MPC_ERR_HIP, "the diff counted %d of %lld tiles", count, d->tiles);
    if (held[0] > static_cast<unsigned long long>(d->tiles - count)) return fail(MPC_ERR_HIP, "the diff held %llu of %lld tiles", held[0], d->tiles - count);
    call.held = static_cast<long long>(held[0]);
    call.held_sse = held[1];
    call.n = count;
    d->changed.resize(static_cast<size_t>(call.n));
    if (call.n > 0) {
        HIP_TRY(hipMemcpyAsync(d->changed.data(), d->d_list, sizeof(int32_t) * static_cast<size_t>(call.n), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return MPC_OK;
}

// 4. - 6. pursue: a key frame straight into the record store, else the packed frame of the listed tiles and its records scattered
mpc_status delta_pursue(mpc_delta* d, hipStream_t s, DeltaCall& call) {
    mpc_context* c = d->ctx;
    const int K = c->K;
    if (!call.through_pack)
        return mpc_encode_tiles_device(c, call.frame, d->width, d->height, call.stride, 0, d->tiles_y, call.quant, d->d_counts, d->d_choices, nullptr,
                                       nullptr, 0, s);
    if (call.n == 0) return MPC_OK;
    const mpc::PackGeometry g = call.g = mpc::pack_geometry(call.n, MPC_DELTA_PACK_ROWS);
    const size_t packed_tc = 3 * static_cast<size_t>(g.rows) * static_cast<size_t>(g.cols);
    uint8_t* d_packed = nullptr;
    const auto layout = [&](char* base) {
        Carve cv{base};
        d_packed = cv.take<uint8_t>(g.bytes);
        call.d_packed_counts = cv.take<uint16_t>(packed_tc + 2);
        call.d_packed_choices = cv.take<mpc_basis_choice>(packed_tc * static_cast<size_t>(K));
        return cv.at;
    };
    if (const mpc_status gs = d->pack.reserve(layout(nullptr), "delta packed frame"); gs != MPC_OK) return gs;
    layout(d->pack.data());
    if (const int e = mpc::launch_tile_pack(call.frame, d->width, d->height, call.stride, d->d_list, call.n, g.rows, g.cols, d_packed, g.stride, s); e != 0)
        return launch_failed(e);
    if (const mpc_status es = mpc_encode_tiles_device(c, d_packed, 8 * g.cols, 8 * g.rows, g.stride, 0, g.rows, call.quant, call.d_packed_counts,
                                                      call.d_packed_choices, nullptr, nullptr, 0, s);
        es != MPC_OK)
        return es;
    if (const int e = mpc::launch_tile_scatter_records(call.d_packed_counts, reinterpret_cast<const uint32_t*>(call.d_packed_choices), d->d_list, call.n,
                                                       K, d->d_counts, reinterpret_cast<uint32_t*>(d->d_choices), d->tiles, d->d_count + 1, s);
        e != 0)
        return launch_failed(e);
    return MPC_OK;
}

extern "C" {

mpc_status mpc_delta_encode(mpc_delta* d, const uint8_t* rgb, size_t row_stride, const double* quant, unsigned flags, int index_interval,
                            uint8_t** bytes, size_t* nbytes, uint8_t** index, size_t* index_bytes, mpc_delta_info* info) {
    return guarded([&]() -> mpc_status {
        if (!d || !rgb || !bytes || !nbytes || !info) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (index_interval >= 0 && (!index || !index_bytes)) return fail(MPC_ERR_ARGUMENT, "null argument");
        unsigned every = 0;
        if (const mpc_status bad = optional_index_interval_of(index_interval, &every)) return bad;
        return delta_call(
            d, rgb, row_stride, quant, flags, false, info,
            [&] {
                *bytes = nullptr;
                *nbytes = 0;
                if (index) *index = nullptr;
                if (index_bytes) *index_bytes = 0;
                d->sent_valid = false;                              // no budget call: what a receiver holds is no longer tracked
            },
            [&](const DeltaCall&, hipStream_t s, const Tuning& tuning) -> mpc_status {
                ContainerMade made;
                if (const mpc_status cs = records_container(d->ctx, tuning, s, d->d_counts, d->d_choices, d->tiles, d->width, d->height, quant, every, &made);
                    cs != MPC_OK)
                    return cs;
                return deliver_container(made, every, bytes, nbytes, index, index_bytes);
            });
    });
}

}  // extern "C"

namespace {
// mpc_delta_encode_patch, and with `every` != 0 mpc_delta_encode_patch_indexed: the container job also leaves the version-1 seek index,
// and a patch whose container has at least max(index_min_bytes, 1) bytes carries it -- byte for byte host_patch.h's patch_add_index
mpc_status encode_patch(mpc_delta* d, const uint8_t* rgb, size_t row_stride, const double* quant, unsigned flags, unsigned every,
                        size_t index_min_bytes, uint8_t** patch, size_t* patch_bytes, mpc_delta_info* info) {
    bool key_patch = false;
    const mpc_status st = delta_call(
        d, rgb, row_stride, quant, flags, false, info,
        [&] {
            *patch = nullptr;
            *patch_bytes = 0;
            d->sent_valid = false;                                  // no budget call: what a receiver holds is no longer tracked
        },
        [&](const DeltaCall& call, hipStream_t s, const Tuning& tuning) -> mpc_status {
            key_patch = call.key || call.n == d->tiles;
            ContainerMade made;
            if (key_patch) {                                        // the whole frame's container from the store
                if (const mpc_status cs =
                        records_container(d->ctx, tuning, s, d->d_counts, d->d_choices, d->tiles, d->width, d->height, quant, every, &made, false);
                    cs != MPC_OK)
                    return cs;
            } else if (call.n > 0) {                                // the packed frame's, from its own counts and records
                if (const mpc_status cs = records_container(d->ctx, tuning, s, call.d_packed_counts, call.d_packed_choices,
                                                            static_cast<long long>(call.g.rows) * call.g.cols, 8 * call.g.cols, 8 * call.g.rows, quant,
                                                            every, &made, false);
                    cs != MPC_OK)
                    return cs;
            }
            // the index goes along unless the patch is too small to gain by it or it says "serial only" (its flags word, bit 0: the
            // host route's, for a code longer than 32 bits)
            const bool indexed = every != 0 && call.n > 0 && made.nbytes >= (index_min_bytes ? index_min_bytes : 1) && made.index.size() >= 16 &&
                                 !(made.index[12] & 1u) && static_cast<uint64_t>(made.index.size()) < (1ULL << 32);
            const uint8_t* index = indexed ? made.index.data() : nullptr;
            const size_t index_bytes = indexed ? made.index.size() : 0;
            const std::string why =
                mpc::patch_make_error(d->width, d->height, key_patch, d->changed.data(), call.n, made.bytes, made.nbytes, index, index_bytes);
            if (!why.empty()) return fail(MPC_ERR_HIP, "the patch: %s", why.c_str());
            const std::vector<uint8_t> blob =
                mpc::patch_make(d->width, d->height, d->calls, key_patch, d->changed.data(), call.n, made.bytes, made.nbytes, index, index_bytes);
            uint8_t* out = static_cast<uint8_t*>(std::malloc(blob.size()));
            if (!out) return fail(MPC_ERR_ALLOC, "no patch");
            std::memcpy(out, blob.data(), blob.size());
            *patch = out;
            *patch_bytes = blob.size();
            return MPC_OK;
        });
    if (st == MPC_OK && key_patch) info->key = 1;                   // every tile listed: sent as a key patch
    return st;
}
}  // namespace

extern "C" {

mpc_status mpc_delta_encode_patch(mpc_delta* d, const uint8_t* rgb, size_t row_stride, const double* quant, unsigned flags, uint8_t** patch,
                                  size_t* patch_bytes, mpc_delta_info* info) {
    return guarded([&]() -> mpc_status {
        if (!d || !rgb || !patch || !patch_bytes || !info) return fail(MPC_ERR_ARGUMENT, "null argument");
        return encode_patch(d, rgb, row_stride, quant, flags, 0, 0, patch, patch_bytes, info);
    });
}

mpc_status mpc_delta_encode_patch_indexed(mpc_delta* d, const uint8_t* rgb, size_t row_stride, const double* quant, unsigned flags,
                                          int index_interval, size_t index_min_bytes, uint8_t** patch, size_t* patch_bytes,
                                          mpc_delta_info* info) {
    return guarded([&]() -> mpc_status {
        if (!d || !rgb || !patch || !patch_bytes || !info) return fail(MPC_ERR_ARGUMENT, "null argument");
        unsigned every = 0;
        if (const mpc_status bad = optional_index_interval_of(index_interval, &every)) return bad;
        return encode_patch(d, rgb, row_stride, quant, flags, every, index_min_bytes, patch, patch_bytes, info);
    });
}

}  // extern "C"
