// mpcodec_rd.cpp -- product: Compression.cpp's -n / -g measurement (Compression.cpp:144-182, :303-350) for one frame at many
// quantiser tables (mpc_rate_distortion[_device], include/mpcodec.h).  A client of the single-device C ABI and of the HIP runtime.
//
// Per level, without the container coming back in: tile encode (mpc_encode_tiles_device, whole frame) on `enc`; then, on `side`
// behind it, the reconstruction error against the frame (mpc_distortion_device: one u64 per level) and the container job
// (mpc_container_job_begin).  Software-pipelined like the multi-GPU lanes (mpcodec_multi.cpp): while level i's pursuit runs on
// 7/8 of the CUs, the host builds level i-1's code tables and level i-2's container is collected; the small kernels of the side
// stream run on the CUs the pursuit leaves free.  Three record buffers, one per container job slot in flight.
// PSNR from the exact integer SSE with calculatePSNR's formula (CompressedImage.cpp:343-357).
#include "../../include/mpcodec.h"
#include "host_codec.h"
#include "mpc_internal.h"

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <new>
#include <vector>

namespace {

constexpr int kSlots = 3;       // levels in flight: encoding, tables being built, container being collected
static_assert(kSlots <= MPC_JOB_SLOTS, "one container job slot per level in flight");

// everything a call owns; released (after the streams drained) on every way out
struct Sweep {
    mpc_context* ctx = nullptr;
    int saved_workgroups = 0;
    bool workgroups_set = false;
    hipStream_t enc = nullptr, side = nullptr;
    hipEvent_t encoded[kSlots] = {};
    uint16_t* d_counts[kSlots] = {};
    mpc_basis_choice* d_choices[kSlots] = {};
    unsigned long long* d_sse = nullptr;
    uint8_t* d_frame = nullptr;          // the host form's upload
    bool jobs_begun = false;
    ~Sweep() {
        if (enc) (void)hipStreamSynchronize(enc);
        if (side) (void)hipStreamSynchronize(side);
        if (jobs_begun)
            for (int slot = 0; slot < kSlots; ++slot) (void)mpc_container_job_cancel(ctx, slot);
        for (int k = 0; k < kSlots; ++k) {
            (void)hipFree(d_counts[k]);
            (void)hipFree(d_choices[k]);
            if (encoded[k]) (void)hipEventDestroy(encoded[k]);
        }
        (void)hipFree(d_sse);
        (void)hipFree(d_frame);
        if (enc) (void)hipStreamDestroy(enc);
        if (side) (void)hipStreamDestroy(side);
        if (workgroups_set) (void)mpc_context_set_tile_encode_workgroups(ctx, saved_workgroups);
    }
};

#define RD_HIP(call)                                                                                   \
    do {                                                                                               \
        const hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) return fail(MPC_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)
#define RD_MPC(call)                              \
    do {                                          \
        const mpc_status s_ = (call);             \
        if (s_ != MPC_OK) return s_;              \
    } while (0)

mpc_status check_args(mpc_context* ctx, const void* frame, int width, int height, const double* quants, int n_levels, size_t* nbytes) {
    if (!ctx) return fail(MPC_ERR_ARGUMENT, "null context");
    if (!frame || !quants || !nbytes) return fail(MPC_ERR_ARGUMENT, "null argument");
    if (n_levels < 1) return fail(MPC_ERR_ARGUMENT, "n_levels = %d, at least one level", n_levels);
    if (width < 1 || height < 1) return fail(MPC_ERR_ARGUMENT, "bad geometry %dx%d", width, height);
    if (static_cast<long long>((width + 7) / 8) * ((height + 7) / 8) * 3 >= (1LL << 31)) return fail(MPC_ERR_ARGUMENT, "frame too large");
    if (mpc_context_device(ctx) < 0) return no_device();
    return MPC_OK;
}

mpc_status sweep(Sweep& w, const uint8_t* d_rgb, int width, int height, const double* quants, int n_levels, size_t* nbytes,
                 unsigned long long* sse, double* psnr, uint8_t** bytes) {
    mpc_context* ctx = w.ctx;
    const int K = mpc_context_K(ctx), tiles_y = (height + 7) / 8;
    const size_t tiles = static_cast<size_t>((width + 7) / 8) * tiles_y, n_tc = tiles * 3;
    const size_t level_quant = 3 * static_cast<size_t>(K);
    RD_HIP(hipStreamCreateWithFlags(&w.enc, hipStreamNonBlocking));
    RD_HIP(hipStreamCreateWithFlags(&w.side, hipStreamNonBlocking));
    const int slots = n_levels < kSlots ? n_levels : kSlots;
    for (int k = 0; k < slots; ++k) {
        RD_HIP(hipEventCreateWithFlags(&w.encoded[k], hipEventDisableTiming));
        RD_HIP(hipMalloc(reinterpret_cast<void**>(&w.d_counts[k]), sizeof(uint16_t) * n_tc));
        RD_HIP(hipMalloc(reinterpret_cast<void**>(&w.d_choices[k]), sizeof(mpc_basis_choice) * n_tc * K));
    }
    RD_HIP(hipMalloc(reinterpret_cast<void**>(&w.d_sse), sizeof(unsigned long long) * n_levels));
    RD_HIP(hipMemsetAsync(w.d_sse, 0, sizeof(unsigned long long) * n_levels, w.side));
    // the pursuits leave one CU in eight to the side stream, unless the caller has chosen a share already
    w.saved_workgroups = mpc_context_tile_encode_workgroups(ctx);
    const int cus = mpc_context_max_waves(ctx) / 12;
    if (w.saved_workgroups == 0 && cus >= 16) {
        RD_MPC(mpc_context_set_tile_encode_workgroups(ctx, cus - cus / 8));
        w.workgroups_set = true;
    }
    std::vector<uint8_t*> out(static_cast<size_t>(n_levels), nullptr);
    struct Containers {                     // collected containers: the caller's only on success
        std::vector<uint8_t*>& v;
        bool keep = false;
        ~Containers() {
            if (!keep)
                for (uint8_t* p : v) mpc_free(p);
        }
    } owned{out};
    auto collect = [&](int level) -> mpc_status {
        RD_MPC(mpc_container_job_collect(ctx, level % kSlots, &out[static_cast<size_t>(level)], &nbytes[level]));
        if (!bytes) {                       // sizes only
            mpc_free(out[static_cast<size_t>(level)]);
            out[static_cast<size_t>(level)] = nullptr;
        }
        return MPC_OK;
    };
    w.jobs_begun = true;
    for (int i = 0; i < n_levels; ++i) {
        const int slot = i % kSlots;
        const double* q = quants + level_quant * static_cast<size_t>(i);
        // slot's records were last read by level i-3's container job, collected in the previous iteration
        RD_MPC(mpc_encode_tiles_device(ctx, d_rgb, width, height, static_cast<size_t>(3) * width, 0, tiles_y, q, w.d_counts[slot],
                                       w.d_choices[slot], nullptr, nullptr, 0, w.enc));
        RD_HIP(hipEventRecord(w.encoded[slot], w.enc));
        RD_HIP(hipStreamWaitEvent(w.side, w.encoded[slot], 0));
        RD_MPC(mpc_distortion_device(ctx, w.d_counts[slot], w.d_choices[slot], q, d_rgb, width, height, w.d_sse + i, nullptr, w.side));
        RD_MPC(mpc_container_job_begin(ctx, slot, w.d_counts[slot], w.d_choices[slot], width, height, q, w.side));
        if (i >= 1) RD_MPC(mpc_container_job_tables(ctx, (i - 1) % kSlots));
        if (i >= 2) RD_MPC(collect(i - 2));
    }
    RD_MPC(mpc_container_job_tables(ctx, (n_levels - 1) % kSlots));
    for (int i = n_levels >= 2 ? n_levels - 2 : 0; i < n_levels; ++i) RD_MPC(collect(i));
    w.jobs_begun = false;
    std::vector<unsigned long long> h_sse(static_cast<size_t>(n_levels));
    RD_HIP(hipMemcpyAsync(h_sse.data(), w.d_sse, sizeof(unsigned long long) * n_levels, hipMemcpyDeviceToHost, w.side));
    RD_HIP(hipStreamSynchronize(w.side));
    for (int i = 0; i < n_levels; ++i) {
        if (sse) sse[i] = h_sse[static_cast<size_t>(i)];
        if (psnr) psnr[i] = mpc::psnr_from_sse(static_cast<double>(h_sse[static_cast<size_t>(i)]), width, height);
        if (bytes) bytes[i] = out[static_cast<size_t>(i)];
    }
    owned.keep = true;
    return MPC_OK;
}

mpc_status rate_distortion(mpc_context* ctx, const uint8_t* frame, bool on_device, int width, int height, const double* quants,
                           int n_levels, size_t* nbytes, unsigned long long* sse, double* psnr, uint8_t** bytes) {
    try {
        RD_MPC(check_args(ctx, frame, width, height, quants, n_levels, nbytes));
        for (int i = 0; i < n_levels; ++i) {
            nbytes[i] = 0;
            if (bytes) bytes[i] = nullptr;
        }
        RD_HIP(hipSetDevice(mpc_context_device(ctx)));
        Sweep w;
        w.ctx = ctx;
        const uint8_t* d_rgb = frame;
        if (!on_device) {
            const size_t frame_bytes = static_cast<size_t>(3) * width * height;
            RD_HIP(hipMalloc(reinterpret_cast<void**>(&w.d_frame), frame_bytes));
            RD_HIP(hipMemcpy(w.d_frame, frame, frame_bytes, hipMemcpyHostToDevice));
            d_rgb = w.d_frame;
        }
        const mpc_status st = sweep(w, d_rgb, width, height, quants, n_levels, nbytes, sse, psnr, bytes);
        if (st != MPC_OK)
            for (int i = 0; i < n_levels; ++i) nbytes[i] = 0;
        return st;
    } catch (const std::bad_alloc&) {
        return fail(MPC_ERR_ALLOC, "out of memory");
    } catch (const std::exception& e) {
        return fail(MPC_ERR_HIP, "%s", e.what());
    }
}

}  // namespace

extern "C" {

mpc_status mpc_rate_distortion(mpc_context* ctx, const uint8_t* rgb, int width, int height, const double* quants, int n_levels,
                               size_t* nbytes, unsigned long long* sse, double* psnr, uint8_t** bytes) {
    return rate_distortion(ctx, rgb, false, width, height, quants, n_levels, nbytes, sse, psnr, bytes);
}

mpc_status mpc_rate_distortion_device(mpc_context* ctx, const uint8_t* d_rgb, int width, int height, const double* quants, int n_levels,
                                      size_t* nbytes, unsigned long long* sse, double* psnr, uint8_t** bytes) {
    return rate_distortion(ctx, d_rgb, true, width, height, quants, n_levels, nbytes, sse, psnr, bytes);
}

}  // extern "C"
