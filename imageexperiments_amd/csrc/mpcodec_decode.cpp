// mpcodec_decode.cpp -- product: tile reconstruction on the device from records (decode_tiles_on_device, which the container
// decoder of mpcodec_decode_seq.cpp ends in, and mpc_decode_tiles_device), the device distortion of the rate-distortion sweep, and
// the "-s" patch statistics.
#include <algorithm>
#include <cstring>
#include <string>

#include "host_codec.h"
#include "host_stats.h"
#include "mpc_internal.h"

// FromCoeffsDynamic + RGBFromYUV for whole tiles on the device.  window: only the tiles a pixel rectangle touches,
// d_rgb then receiving the rectangle alone.  view (with a window): the first view->steps records, reduced (mp_decode_view_kernel)
mpc_status decode_tiles_on_device(mpc_context* c, const uint16_t* d_counts, const uint32_t* d_choices, const double* d_quant,
                                  int K, int width, int height, uint8_t* d_rgb, int* d_flag, void* stream, const mpc::DecodeWindow* window,
                                  const mpc::DecodeView* view) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int), s));
    mpc::DecodeParams p{};
    p.counts = d_counts;
    p.choices = d_choices;
    p.quant = d_quant;
    p.K = K;
    p.width = width;
    p.height = height;
    p.tiles_x = (width + 7) / 8;
    p.tiles_y = (height + 7) / 8;
    p.rgb = d_rgb;
    p.error_flag = d_flag;
    p.fast = c->fast ? 1 : 0;
    if (view && !window) return fail(MPC_ERR_ARGUMENT, "a view needs its window");
    const int err = view     ? mpc::launch_decode_view(dict_device(c), p, *window, *view, stream)
                    : window ? mpc::launch_decode_window(dict_device(c), p, *window, stream)
                             : mpc::launch_decode(dict_device(c), p, stream);
    if (err != 0) return launch_failed(err);
    return MPC_OK;
}

namespace {
// the context's own error word (mpc_decode_tiles_device)
mpc_status context_flag(mpc_context* c) {
    if (!c->d_flag) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->d_flag), sizeof(int)));
    return MPC_OK;
}
}  // namespace

extern "C" {

mpc_status mpc_decode_tiles_device(mpc_context* c, const uint16_t* d_counts, const mpc_basis_choice* d_choices,
                                   const double* quant, int width, int height, uint8_t* d_rgb, void* stream) {
    if (!c || !d_counts || !d_choices || !d_rgb) return fail(MPC_ERR_ARGUMENT, "null argument");
    if (c->device < 0) return fail(MPC_ERR_NO_DEVICE, "context was created without a device");
    if (width < 1 || height < 1) return fail(MPC_ERR_ARGUMENT, "bad geometry");
    HIP_TRY(hipSetDevice(c->device));
    if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
    if (const mpc_status fs = context_flag(c); fs != MPC_OK) return fs;
    CallQuant cq;
    if (const mpc_status qs = call_quant(c, quant, static_cast<hipStream_t>(stream), &cq); qs != MPC_OK) return qs;
    return decode_tiles_on_device(c, d_counts, reinterpret_cast<const uint32_t*>(d_choices), cq.d_q, c->K, width, height, d_rgb,
                                  c->d_flag, stream);
}

// the decoder's reconstruction compared with the original frame on the device (mp_distortion_kernel); the quantiser steps are
// the container header's (mpc::header_quant), not the encoder's doubles
mpc_status mpc_distortion_device(mpc_context* c, const uint16_t* d_counts, const mpc_basis_choice* d_choices, const double* quant,
                                 const uint8_t* d_rgb, int width, int height, unsigned long long* d_sse, uint32_t* d_tile_sse,
                                 void* stream) {
    return guarded([&]() -> mpc_status {
    if (!c || !d_counts || !d_choices || !d_rgb || !d_sse) return fail(MPC_ERR_ARGUMENT, "null argument");
    if (c->device < 0) return no_device();
    if (width < 1 || height < 1) return fail(MPC_ERR_ARGUMENT, "bad geometry %dx%d", width, height);
    const long long tiles = static_cast<long long>((width + 7) / 8) * ((height + 7) / 8);
    if (tiles * 3 >= (1LL << 31)) return fail(MPC_ERR_ARGUMENT, "frame too large");
    HIP_TRY(hipSetDevice(c->device));
    if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
    CallQuant cq;
    if (const mpc_status qs = header_quant_device(c, quant, static_cast<hipStream_t>(stream), &cq); qs != MPC_OK) return qs;
    mpc::DistortionParams p{};
    p.counts = d_counts;
    p.choices = reinterpret_cast<const uint32_t*>(d_choices);
    p.quant = cq.d_q;
    p.K = c->K;
    p.width = width;
    p.height = height;
    p.tiles_x = (width + 7) / 8;
    p.tiles_y = (height + 7) / 8;
    p.original = d_rgb;
    p.sse = d_sse;
    p.tile_sse = d_tile_sse;
    p.fast = c->fast ? 1 : 0;
    const int err = mpc::launch_distortion(dict_device(c), p, stream);
    if (err != 0) return launch_failed(err);
    return MPC_OK;
    });
}

// ---- "-s" patch statistics (Compression.cpp:200-302) ----
struct mpc_patch_stats {
    mpc_context* ctx;
    mpc::PatchStats stats;
    std::vector<uint8_t> mosaic;
    std::vector<uint16_t> counts;
    std::vector<uint32_t> choices;
    mpc_patch_stats(mpc_context* c, unsigned seed) : ctx(c), stats(c->K, c->block_size, seed) {}
};

mpc_status mpc_patch_stats_create(mpc_context* c, unsigned seed, mpc_patch_stats** out) {
    if (!c || !out) return fail(MPC_ERR_ARGUMENT, "null argument");
    if (c->device < 0) return no_device();
    try {
        *out = new mpc_patch_stats(c, seed);
    } catch (const std::bad_alloc&) { return fail(MPC_ERR_ALLOC, "out of memory"); }
    return MPC_OK;
}

void mpc_patch_stats_destroy(mpc_patch_stats* s) { delete s; }

mpc_status mpc_patch_stats_add_image(mpc_patch_stats* s, const uint8_t* rgb, int width, int height, int patches) {
    return guarded([&]() -> mpc_status {
    if (!s || !rgb) return fail(MPC_ERR_ARGUMENT, "null argument");
    const int bs = s->stats.block_size, K = s->stats.K;
    if (width < bs || height < bs || patches <= 0) return MPC_OK;            // Compression.cpp:233-236
    if (width == bs || height == bs) return fail(MPC_ERR_ARGUMENT, "image of exactly one block: rand() %% 0 in the reference");
    std::vector<int> xs, ys;
    s->stats.sample_origins(width, height, patches, xs, ys);
    // the patches as the tiles of a one-tile-high mosaic: tile p = patch p (tile order tx*1 + 0)
    const size_t row = static_cast<size_t>(patches) * bs * 3;
    s->mosaic.resize(row * bs);
    for (int p = 0; p < patches; ++p)
        for (int dy = 0; dy < bs; ++dy)
            std::memcpy(s->mosaic.data() + dy * row + static_cast<size_t>(p) * bs * 3,
                        rgb + 3 * (static_cast<size_t>(ys[p] + dy) * width + xs[p]), static_cast<size_t>(bs) * 3);
    s->counts.resize(static_cast<size_t>(patches) * 3);
    s->choices.resize(static_cast<size_t>(patches) * 3 * K);
    const std::vector<double> ones(3 * static_cast<size_t>(K), 1.0);          // Compression.cpp:221-225
    const mpc_status st = mpc_encode_tiles(s->ctx, s->mosaic.data(), patches * bs, bs, row, 0, 1, ones.data(), s->counts.data(),
                                           reinterpret_cast<mpc_basis_choice*>(s->choices.data()), nullptr, nullptr);
    if (st != MPC_OK) return st;
    s->stats.accumulate(s->counts.data(), s->choices.data(), patches);
    return MPC_OK;
    });
}

mpc_status mpc_patch_stats_read(const mpc_patch_stats* s, double* out) {
    if (!s || !out) return fail(MPC_ERR_ARGUMENT, "null argument");
    const int K = s->stats.K;
    for (int ch = 0; ch < 3; ++ch)
        for (int kind = 0; kind < 2; ++kind)
            for (int i = 0; i < K; ++i) {
                const mpc::RunningStat& r = kind == 0 ? s->stats.coeff[ch][i] : s->stats.select[ch][i];
                double* o = out + ((static_cast<size_t>(ch) * 2 + kind) * K + i) * 5;
                o[0] = r.N; o[1] = r.min; o[2] = r.max; o[3] = r.mean; o[4] = r.sumSq;
            }
    return MPC_OK;
}

mpc_status mpc_patch_stats_report(const mpc_patch_stats* s, char** text, size_t* nbytes) {
    return guarded([&]() -> mpc_status {
    if (!s || !text || !nbytes) return fail(MPC_ERR_ARGUMENT, "null argument");
    const std::string r = s->stats.report();
    char* p = static_cast<char*>(std::malloc(r.size() + 1));
    if (!p) return fail(MPC_ERR_ALLOC, "out of memory");
    std::memcpy(p, r.c_str(), r.size() + 1);
    *text = p;
    *nbytes = r.size();
    return MPC_OK;
    });
}

int mpc_format_double(double v, char* buf, int cap) {
    const std::string t = mpc::format_double(v);
    if (!buf || cap <= static_cast<int>(t.size())) return -1;
    std::memcpy(buf, t.c_str(), t.size() + 1);
    return static_cast<int>(t.size());
}

double mpc_psnr(const uint8_t* original, const uint8_t* decoded, int width, int height) {
    return mpc::psnr(original, decoded, width, height);
}

}  // extern "C"
