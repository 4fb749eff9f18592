// mpc_delta_session.h -- product: the delta encoder's session and the driver of one call, shared by the translation units that add a
// kind of call to it: mpcodec_delta.cpp (mpc_delta_encode, mpc_delta_encode_patch[_indexed]) and mpcodec_rate.cpp
// (mpc_delta_encode_patch_budget).  The stages are mpcodec_delta.cpp's.
#pragma once

#include <cstring>

#include "host_delta.h"
#include "mpc_internal.h"

struct mpc_delta {
    mpc_context* ctx = nullptr;
    int width = 0, height = 0, tiles_y = 0;
    long long tiles = 0;
    // grow-only, all of it: `store` is sized once (the geometry is the session's), the others by the largest call so far
    GrowBuffer store{GrowBuffer::kDevice};      // kept frame | counts | records | list | count, error word | the diff's scratch
    GrowBuffer upload{GrowBuffer::kDevice};     // a host frame's tight copy
    GrowBuffer pack{GrowBuffer::kDevice};       // packed frame | its counts | its records
    GrowBuffer rate{GrowBuffer::kDevice};       // budget calls (mpcodec_rate.cpp): the sent map and the per-tile scratch, sized once
    GrowBuffer pack_rate{GrowBuffer::kDevice};  // ... the candidates' packed frame, its records and profile, a probe's cut records
    hipStream_t stream = nullptr;
    uint8_t* d_kept = nullptr;
    uint16_t* d_counts = nullptr;
    mpc_basis_choice* d_choices = nullptr;
    int32_t* d_list = nullptr;
    int32_t* d_count = nullptr;                 // [2]: the diff's count, the scatter's error word
    void* d_scratch = nullptr;
    // the last successful call: what the records in `store` were pursued with
    bool valid = false, fast = false;
    std::vector<double> quant;
    bool changed_all = false;                   // the last call's list is every tile
    std::vector<int32_t> changed;               // else this
    mpc_delta_info info{};
    uint32_t calls = 0;                         // successful calls of either kind so far: the next patch's sequence
    // a delta stream to a byte budget: what the receiver holds of each tile after the last successful budget call
    bool sent_valid = false;                    // the map at d_sent (in `rate`) describes the receiver
    const uint8_t* d_sent = nullptr;
    long long owed = 0;                         // tiles owed after the last successful budget call
    // mpc_delta_set_emphasis: the map budget calls weigh the tiles with; it says nothing about the receiver, so it outlives a failed call
    GrowBuffer emphasis{GrowBuffer::kDevice};   // [tiles]
    bool has_emphasis = false;
    // mpc_delta_set_tolerance: 0 = any differing byte is a change (mp_tile_diff_kernel), else mp_tile_diff_tol_kernel and the kept copy
    // is the composite.  Like the emphasis map it is the caller's wish, not the receiver's state, and outlives a failed call
    uint32_t tolerance = 0;
    GrowBuffer held_totals{GrowBuffer::kDevice};// [2] of a tolerant diff: held tiles, the sum of their sse; reserved by the first one
    long long held = 0;                         // the last successful call's
    uint64_t held_sse = 0;
    ~mpc_delta() {
        if (stream) {
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
    }
};

#pragma GCC visibility push(hidden)

struct DeltaCall {                              // what the stages of one call hand on
    const double* quant = nullptr;              // the caller's table, NULL = the context's
    unsigned flags = 0;
    bool key = false, through_pack = false;
    const uint8_t* frame = nullptr;             // the frame on the device and its stride
    size_t stride = 0;
    long long n = 0;                            // tiles listed
    long long held = 0;                         // a tolerant diff's held tiles and the sum of their sse
    uint64_t held_sse = 0;
    mpc::PackGeometry g{0, 0, 0, 0};            // through_pack && n > 0: the packed frame's geometry, its records in d->pack
    uint16_t* d_packed_counts = nullptr;
    mpc_basis_choice* d_packed_choices = nullptr;
};

// 1. the frame on the device
mpc_status delta_frame(mpc_delta* d, const uint8_t* rgb, size_t row_stride, hipStream_t s, DeltaCall& call);
// 2., 3. the changed tiles: all of them for a key frame, else the diff's list; the kept copy becomes this frame -- with a tolerance the
// composite: this frame in the listed tiles, what it was in every other
mpc_status delta_list(mpc_delta* d, hipStream_t s, DeltaCall& call);
// 4. - 6. pursue: a key frame straight into the record store, else the packed frame of the listed tiles and its records scattered
mpc_status delta_pursue(mpc_delta* d, hipStream_t s, DeltaCall& call);

// One call of any kind.  The caller has checked its own pointers; here the refusals all share, then -- behind `clear`, which empties
// the caller's outputs -- the three shared stages, `finish` (the fourth stage and the caller's result), and the session's new state.
// force_key: the caller's own reason for a key frame
template <class Clear, class Finish>
mpc_status delta_call(mpc_delta* d, const uint8_t* rgb, size_t row_stride, const double* quant, unsigned flags, bool force_key,
                      mpc_delta_info* info, Clear&& clear, Finish&& finish) {
    if (flags & ~(MPC_DELTA_KEY | MPC_DELTA_DEVICE_PIXELS | MPC_DELTA_PACK_ALWAYS)) return fail(MPC_ERR_ARGUMENT, "flags 0x%x", flags);
    mpc_context* c = d->ctx;
    const int K = c->K;
    const size_t row = 3 * static_cast<size_t>(d->width);
    if (row_stride != 0 && row_stride < row) return fail(MPC_ERR_ARGUMENT, "row_stride %zu for %d pixels", row_stride, d->width);
    if (c->device < 0) return no_device();
    std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
    for (int k = 0; k < mpc_context::kSeqSlots; ++k)
        if (c->jobs[k] && c->jobs[k]->stage != 0) return fail(MPC_ERR_ARGUMENT, "container job slot %d is busy", k);
    // behind the checks: whatever fails from here on leaves a session whose next call is a key frame
    clear();
    struct Session {
        mpc_delta* d;
        bool keep = false;
        ~Session() {
            if (keep) return;
            d->valid = false;
            d->sent_valid = false;
            d->changed_all = false;
            d->changed.clear();
            d->info = mpc_delta_info{};
            d->held = 0;
            d->held_sse = 0;
        }
    } session{d};
    HIP_TRY(hipSetDevice(c->device));
    const Tuning tuning = read_tuning();
    const double* table = quant ? quant : c->quant.data();
    const size_t table_bytes = sizeof(double) * 3 * static_cast<size_t>(K);
    DeltaCall call;
    call.quant = quant;
    call.flags = flags;
    call.key = !d->valid || force_key || (flags & MPC_DELTA_KEY) || d->fast != c->fast || d->quant.size() != 3 * static_cast<size_t>(K) ||
               std::memcmp(d->quant.data(), table, table_bytes) != 0;
    call.through_pack = !call.key || (flags & MPC_DELTA_PACK_ALWAYS);
    hipStream_t s = d->stream;
    struct Drain {                                              // whatever happens, nothing of this call is left running
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{s};
    if (const mpc_status st = delta_frame(d, rgb, row_stride, s, call); st != MPC_OK) return st;
    if (const mpc_status st = delta_list(d, s, call); st != MPC_OK) return st;
    if (const mpc_status st = delta_pursue(d, s, call); st != MPC_OK) return st;
    if (const mpc_status st = finish(call, s, tuning); st != MPC_OK) return st;
    d->valid = true;
    d->fast = c->fast;
    d->quant.assign(table, table + 3 * static_cast<size_t>(K));
    d->changed_all = call.key;
    d->info = mpc_delta_info{static_cast<int>(d->tiles), static_cast<int>(call.n), call.key ? 1 : 0};
    d->held = call.held;
    d->held_sse = call.held_sse;
    ++d->calls;
    *info = d->info;
    session.keep = true;
    return MPC_OK;
}

#pragma GCC visibility pop
