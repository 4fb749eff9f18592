// mpcodec_debug.cpp -- product: the mpc_debug_* entry points and mpc_filter_tiles (include/mpcodec.h, "test entry points").
// They exist for the tests of the pursuit screen's tables (tests/test_screen_cases.py, tests/test_gpu_screen_tables.py): the
// resident Gram table, the uploaded split-bf16 filter tiles and the bound of the MFMA approximations decide nothing by
// themselves, so no record can show that they are right; mpc_debug_track_probe_device, the kernel's key tracking by its definition
// and grouped on given bit patterns (tests/test_gpu_track_keys.py); and mpc_debug_container_index_device, the device scan of the seek index
// with its segment and window sizes given, so that a test can make chains cross windows on a small container
// (tests/test_gpu_index_scan.py); and mpc_debug_pair_scratch, which fills and reads the pursuit kernel's per-wave pair scratch
// (kept approximations, bookkeeping word, bound) around a calc_mp call (tests/test_gpu_pair_drift.py).  Nothing here is on a product path; every entry validates its arguments
// before it touches memory.
#include "../../include/mpcodec.h"
#include "mpc_internal.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

namespace {

// null context -> argument error, host-only context -> no device: the order of the rest of the ABI
mpc_status need_device(const mpc_context* c) {
    if (!c) return fail(MPC_ERR_ARGUMENT, "null context");
    if (c->device < 0 || !c->dd) return fail(MPC_ERR_NO_DEVICE, "context was created without a device");
    return MPC_OK;
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

extern "C" {

mpc_status mpc_debug_copy_gram_device(mpc_context* c, int channel, int sel_begin, int sel_count, int col_begin, int col_count,
                                      float* d_out, void* stream) {
    if (const mpc_status st = need_device(c); st != MPC_OK) return st;
    const DeviceDict& d = *c->dd;
    const long long n_sel = d.num_base + d.detail_rows, stride = static_cast<long long>(d.num_base) * 64;
    if (channel < 0 || channel > 2) return fail(MPC_ERR_ARGUMENT, "channel must be 0 ... 2");
    if (!d_out) return fail(MPC_ERR_ARGUMENT, "null output");
    if (sel_begin < 0 || sel_count < 1 || sel_begin > n_sel - sel_count || col_begin < 0 || col_count < 1 || col_begin > stride - col_count)
        return fail(MPC_ERR_ARGUMENT, "rectangle outside the Gram table (%lld x %lld)", n_sel, stride);
    HIP_TRY(hipSetDevice(c->device));
    if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
    const float* src = d.d_gram + (static_cast<long long>(channel) * n_sel + sel_begin) * stride + col_begin;
    HIP_TRY(hipMemcpy2DAsync(d_out, sizeof(float) * col_count, src, sizeof(float) * stride, sizeof(float) * col_count,
                             static_cast<size_t>(sel_count), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return MPC_OK;
}

mpc_status mpc_debug_gram_device(const double* d_base, const double* d_detail, const int32_t* d_block_rows, const int32_t* d_block_row_off,
                                 const uint8_t* d_shadow, int num_base, int n_sel, float* d_gram, void* stream) {
    if (!d_base || !d_detail || !d_block_rows || !d_block_row_off || !d_shadow || !d_gram) return fail(MPC_ERR_ARGUMENT, "null pointer");
    if (num_base < 1 || num_base > 512 || n_sel < num_base || n_sel > (1 << 20)) return fail(MPC_ERR_ARGUMENT, "bad num_base / n_sel");
    if (!aligned16(d_gram)) return fail(MPC_ERR_ARGUMENT, "d_gram must be 16-byte aligned");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return fail(MPC_ERR_NO_DEVICE, "no device");
    if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
    if (const int err = mpc::launch_gram(d_base, d_detail, d_block_rows, d_block_row_off, d_shadow, d_gram, num_base, n_sel,
                                         static_cast<long long>(num_base) * 64, stream))
        return launch_failed(err);
    return MPC_OK;
}

mpc_status mpc_debug_copy_filter_tiles(mpc_context* c, int channel, int block, uint16_t* host_out) {
    if (const mpc_status st = need_device(c); st != MPC_OK) return st;
    const DeviceDict& d = *c->dd;
    if (channel < -1 || channel > 2) return fail(MPC_ERR_ARGUMENT, "channel must be -1 (base tiles) or 0 ... 2");
    if (channel >= 0 && (block < 0 || block >= d.num_base)) return fail(MPC_ERR_ARGUMENT, "block must be 0 ... %d", d.num_base - 1);
    if (!host_out) return fail(MPC_ERR_ARGUMENT, "null output");
    HIP_TRY(hipSetDevice(c->device));
    const size_t per_block = static_cast<size_t>(mpc::kBlockFilterTiles) * mpc::kFilterTileHalves;
    const uint16_t* src = channel < 0 ? d.d_base_t1 : d.d_detail_t1 + (static_cast<size_t>(channel) * d.num_base + block) * per_block;
    const size_t halves = channel < 0 ? static_cast<size_t>(mpc::kBaseFilterTiles) * mpc::kFilterTileHalves : per_block;
    HIP_TRY(hipMemcpy(host_out, src, sizeof(uint16_t) * halves, hipMemcpyDeviceToHost));
    return MPC_OK;
}

mpc_status mpc_filter_tiles(const double* rows, int nrows, int tiles, int k_order, uint16_t* out, uint8_t* shadow) {
    if (!rows || !out) return fail(MPC_ERR_ARGUMENT, "null pointer");
    if (tiles < 1 || tiles > 64 || nrows < 0 || nrows > 16 * tiles) return fail(MPC_ERR_ARGUMENT, "nrows must be 0 ... 16 * tiles, tiles 1 ... 64");
    if (k_order != 0 && k_order != 1) return fail(MPC_ERR_ARGUMENT, "k_order must be 0 or 1");
    return guarded([&]() {
        std::vector<uint8_t> sh;
        const std::vector<uint16_t> t = mpc::filter_tiles(rows, nrows, tiles, k_order, &sh);
        std::memcpy(out, t.data(), sizeof(uint16_t) * t.size());
        if (shadow && nrows > 0) std::memcpy(shadow, sh.data(), static_cast<size_t>(nrows));
        return MPC_OK;
    });
}

mpc_status mpc_debug_container_index_device(mpc_context* c, const uint8_t* bytes, size_t nbytes, int interval, int segment_bits, int window_bits,
                                            uint8_t** index, size_t* index_bytes, int* route) {
    return container_index_on_device(c, bytes, nbytes, interval, 0, segment_bits, window_bits, index, index_bytes, route);
}

mpc_status mpc_debug_screen_probe_device(mpc_context* c, int channel, int block, const double* d_vectors, int n, float* d_approx,
                                         float* d_bound, void* stream) {
    if (const mpc_status st = need_device(c); st != MPC_OK) return st;
    const DeviceDict& d = *c->dd;
    if (channel < 0 || channel > 2) return fail(MPC_ERR_ARGUMENT, "channel must be 0 ... 2");
    if (block < 0 || block >= d.num_base) return fail(MPC_ERR_ARGUMENT, "block must be 0 ... %d", d.num_base - 1);
    if (n < 1 || n > 16) return fail(MPC_ERR_ARGUMENT, "n must be 1 ... 16");
    if (!d_vectors || !d_approx || !d_bound) return fail(MPC_ERR_ARGUMENT, "null pointer");
    if (!aligned16(d_vectors) || !aligned16(d_approx)) return fail(MPC_ERR_ARGUMENT, "d_vectors and d_approx must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
    const uint16_t* block_tiles =
        d.d_detail_t1 + (static_cast<size_t>(channel) * d.num_base + block) * mpc::kBlockFilterTiles * mpc::kFilterTileHalves;
    if (const int err = mpc::launch_screen_probe(d.d_base_t1, block_tiles, d_vectors, n, d_approx, d_bound, stream)) return launch_failed(err);
    return MPC_OK;
}

mpc_status mpc_debug_pair_scratch(mpc_context* c, int wave_begin, int wave_count, int fill, uint32_t fill_word, float* host_p,
                                  uint32_t* host_meta, float* host_e) {
    if (const mpc_status st = need_device(c); st != MPC_OK) return st;
    DeviceDict& d = *c->dd;
    // the scratch is [workgroups * kWavesMax][16 slots][kMaxPairs]: the wave count follows from the size of the bounds
    const size_t per_wave = static_cast<size_t>(16) * mpc::kMaxPairs;
    const long long waves = static_cast<long long>(mpc::pursuit_scratch_bounds(d.workgroups) / per_wave);
    if (fill != 0 && fill != 1) return fail(MPC_ERR_ARGUMENT, "fill must be 0 or 1");
    if (!host_p || !host_meta || !host_e) return fail(MPC_ERR_ARGUMENT, "null output");
    if (wave_begin < 0 || wave_count < 1 || wave_begin > waves - wave_count)
        return fail(MPC_ERR_ARGUMENT, "waves outside the scratch (%lld)", waves);
    HIP_TRY(hipSetDevice(c->device));
    std::lock_guard<std::mutex> hold(d.launch_lock);          // no pursuit is enqueued meanwhile ...
    HIP_TRY(hipDeviceSynchronize());                          // ... and none is running
    const size_t first = static_cast<size_t>(wave_begin) * per_wave, count = static_cast<size_t>(wave_count) * per_wave;
    float* const p = d.pair_p + first * 64;
    unsigned* const meta = d.pair_meta + first * 2;
    float* const e = d.pair_e + first;
    if (fill) {
        HIP_TRY(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(p), static_cast<int>(fill_word), count * 64));
        HIP_TRY(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(meta), static_cast<int>(fill_word), count * 2));
        HIP_TRY(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(e), static_cast<int>(fill_word), count));
    }
    HIP_TRY(hipMemcpy(host_p, p, sizeof(float) * count * 64, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_meta, meta, sizeof(unsigned) * count * 2, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_e, e, sizeof(float) * count, hipMemcpyDeviceToHost));
    return MPC_OK;
}

mpc_status mpc_debug_track_probe_device(mpc_context* c, const uint32_t* d_row_bits, const uint32_t* d_pair_bits, float bound, int rows,
                                        int pair, uint32_t* d_out, void* stream) {
    if (const mpc_status st = need_device(c); st != MPC_OK) return st;
    if (!d_row_bits || !d_pair_bits || !d_out) return fail(MPC_ERR_ARGUMENT, "null pointer");
    if (!aligned16(d_row_bits) || !aligned16(d_pair_bits)) return fail(MPC_ERR_ARGUMENT, "d_row_bits and d_pair_bits must be 16-byte aligned");
    if (rows < 1 || rows > 64) return fail(MPC_ERR_ARGUMENT, "rows must be 1 ... 64");
    if (pair < 0 || pair >= mpc::kMaxPairs) return fail(MPC_ERR_ARGUMENT, "pair must be 0 ... %d", mpc::kMaxPairs - 1);
    HIP_TRY(hipSetDevice(c->device));
    if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
    if (const int err = mpc::launch_track_probe(d_row_bits, d_pair_bits, bound, rows, pair, d_out, stream)) return launch_failed(err);
    return MPC_OK;
}

}  // extern "C"
