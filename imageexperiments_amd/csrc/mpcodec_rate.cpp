// mpcodec_rate.cpp -- product: a delta stream to a byte budget (include/mpcodec.h, "rate"; DESIGN.md 4, "Delta stream to a byte
// budget"): the host definitions' C entry points, the kernels of mp_rate.hip on the caller's buffers, and the session's budget call:
// mpc_delta_encode_patch's stages up to the records, then the candidates (changed + owed), their packed frame with its records out
// of the store, the full container with its seek index, and mpc_encode_image_budget's bisection with the floor allocation, every
// probe a gather of the sent candidates cut to their depths and one container job.
#include <cstring>
#include <string>

#include "host_budget.h"
#include "host_delta.h"
#include "host_patch.h"
#include "host_rate.h"
#include "mpc_delta_session.h"

extern "C" {

mpc_status mpc_owed_tiles(const uint8_t* sent, const uint16_t* counts, long long tiles, int K, const int32_t* changed, int n_changed,
                          int32_t* candidates, uint8_t* floor, uint8_t* must, int* n) {
    return guarded([&]() -> mpc_status {
        if (!sent || !counts || !n || (n_changed > 0 && !changed)) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (tiles < 0 || tiles >= (1LL << 31) || K < 1 || K > MPC_MAX_K || n_changed < 0 || n_changed > tiles)
            return fail(MPC_ERR_ARGUMENT, "tiles %lld, K %d, %d changed", tiles, K, n_changed);
        for (int k = 0; k < n_changed; ++k)
            if (changed[k] < 0 || changed[k] >= tiles || (k > 0 && changed[k] <= changed[k - 1]))
                return fail(MPC_ERR_ARGUMENT, "the changed tiles: ascending, distinct and inside the frame");
        *n = static_cast<int>(mpc::owed_tiles(sent, counts, tiles, K, changed, n_changed, candidates, floor, must));
        return MPC_OK;
    });
}

mpc_status mpc_budget_allocate_floor(const uint32_t* profile, const uint16_t* counts, const uint8_t* floor, const uint8_t* must, long long n,
                                     int K, const uint32_t* weights, int j, uint8_t* depth, uint16_t* out_counts, uint8_t* send,
                                     uint64_t* totals) {
    return guarded([&]() -> mpc_status {
        if (!profile || !counts || !weights || !totals) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (n < 0 || K < 1 || K > MPC_MAX_K || j < 0 || j >= mpc::kBudgetLambdas) return fail(MPC_ERR_ARGUMENT, "tiles %lld, K %d, multiplier %d", n, K, j);
        mpc::budget_allocate_floor(profile, counts, floor, must, n, K, weights, j, depth, out_counts, send, totals);
        return MPC_OK;
    });
}

mpc_status mpc_owed_tiles_device(mpc_context* c, const uint8_t* d_sent, const uint16_t* d_counts, long long tiles, uint8_t* d_flags,
                                 uint8_t* d_floor, uint8_t* d_must, int32_t* d_list, int32_t* d_count, void* stream) {
    return guarded([&]() -> mpc_status {
        if (!c || !d_sent || !d_counts || !d_flags || !d_floor || !d_must || !d_list || !d_count) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (c->device < 0) return no_device();
        if (tiles < 1 || tiles >= (1LL << 31)) return fail(MPC_ERR_ARGUMENT, "tiles %lld", tiles);
        std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
        HIP_TRY(hipSetDevice(c->device));
        if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
        if (const mpc_status gs = c->delta_scratch.reserve(mpc::tile_diff_scratch_bytes(tiles), "diff scratch"); gs != MPC_OK) return gs;
        if (const int e = mpc::launch_owed_flags(d_sent, d_counts, tiles, c->K, d_flags, d_floor, d_must, stream); e != 0) return launch_failed(e);
        if (const int e = mpc::launch_tile_flags_list(d_flags, tiles, mpc::tile_diff_block_live(c->delta_scratch.data(), tiles), d_list, d_count, stream);
            e != 0)
            return launch_failed(e);
        return MPC_OK;
    });
}

mpc_status mpc_gather_records_device(mpc_context* c, const uint16_t* d_counts, const mpc_basis_choice* d_choices, int tiles, const int32_t* d_list,
                                     int m, const int32_t* d_idx, const uint8_t* d_depth, int n, int rows, uint16_t* d_packed_counts,
                                     mpc_basis_choice* d_packed_choices, void* stream) {
    return guarded([&]() -> mpc_status {
        if (!c || !d_counts || !d_choices || !d_list || !d_packed_counts || !d_packed_choices) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (c->device < 0) return no_device();
        if (n < 1 || m < 1 || tiles < 1 || rows < 1 || (!d_idx && n > m)) return fail(MPC_ERR_ARGUMENT, "n %d of %d listed, tiles %d, rows %d", n, m, tiles, rows);
        const mpc::PackGeometry g = mpc::pack_geometry(n, rows);
        const long long padded = static_cast<long long>(g.rows) * g.cols;
        if (padded >= (1LL << 31) / (3 * MPC_MAX_K)) return fail(MPC_ERR_ARGUMENT, "bad geometry");
        HIP_TRY(hipSetDevice(c->device));
        if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
        if (const mpc_status fs = crop_flag(c); fs != MPC_OK) return fs;
        mpc::GatherParams p{};
        p.counts = d_counts;
        p.choices = reinterpret_cast<const uint32_t*>(d_choices);
        p.tiles = tiles;
        p.list = d_list;
        p.m = m;
        p.idx = d_idx;
        p.depth = d_depth;
        p.n = n;
        p.padded = padded;
        p.K = c->K;
        p.out_counts = d_packed_counts;
        p.out_choices = reinterpret_cast<uint32_t*>(d_packed_choices);
        p.error = c->d_crop_flag;
        if (const int e = mpc::launch_gather_records(p, stream); e != 0) return launch_failed(e);
        return MPC_OK;
    });
}

mpc_status mpc_budget_allocate_floor_emphasis(const uint32_t* profile, const uint16_t* counts, const uint8_t* floor, const uint8_t* must,
                                              const uint8_t* emphasis, const int32_t* list, long long tiles, long long n, int K,
                                              const uint32_t* weights, int j, uint8_t* depth, uint16_t* out_counts, uint8_t* send, uint64_t* totals) {
    return guarded([&]() -> mpc_status {
        if (!profile || !counts || !weights || !totals) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (n < 0 || K < 1 || K > MPC_MAX_K || j < 0 || j >= mpc::kBudgetLambdas) return fail(MPC_ERR_ARGUMENT, "tiles %lld, K %d, multiplier %d", n, K, j);
        if (emphasis && (tiles < 1 || (!list && n > tiles))) return fail(MPC_ERR_ARGUMENT, "%lld candidates, an emphasis map of %lld tiles", n, tiles);
        mpc::budget_allocate_floor_emphasis(profile, counts, floor, must, emphasis, list, tiles, n, K, weights, j, depth, out_counts, send, totals);
        return MPC_OK;
    });
}

mpc_status mpc_budget_allocate_floor_device(mpc_context* c, const uint32_t* d_profile, const uint16_t* d_counts, const uint8_t* d_floor,
                                            const uint8_t* d_must, long long n, const uint32_t* weights, int j, uint8_t* d_depth,
                                            uint16_t* d_out_counts, uint8_t* d_send, unsigned long long* d_totals, void* stream) {
    return mpc_budget_allocate_floor_emphasis_device(c, d_profile, d_counts, d_floor, d_must, nullptr, nullptr, 0, n, weights, j, d_depth, d_out_counts,
                                                     d_send, d_totals, stream);
}

mpc_status mpc_budget_allocate_floor_emphasis_device(mpc_context* c, const uint32_t* d_profile, const uint16_t* d_counts, const uint8_t* d_floor,
                                                     const uint8_t* d_must, const uint8_t* d_emphasis, const int32_t* d_list, long long tiles,
                                                     long long n, const uint32_t* weights, int j, uint8_t* d_depth, uint16_t* d_out_counts,
                                                     uint8_t* d_send, unsigned long long* d_totals, void* stream) {
    return guarded([&]() -> mpc_status {
        if (!c || !d_profile || !d_counts || !weights || !d_depth || !d_out_counts || !d_send || !d_totals) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (c->device < 0) return no_device();
        if (n < 1 || n * 3 >= (1LL << 31) || j < 0 || j >= mpc::kBudgetLambdas) return fail(MPC_ERR_ARGUMENT, "tiles %lld, multiplier %d", n, j);
        if (d_emphasis && (tiles < 1 || tiles >= (1LL << 31) || (!d_list && n > tiles)))
            return fail(MPC_ERR_ARGUMENT, "%lld candidates, an emphasis map of %lld tiles", n, tiles);
        HIP_TRY(hipSetDevice(c->device));
        if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
        hipStream_t s = static_cast<hipStream_t>(stream);
        HIP_TRY(hipMemsetAsync(d_totals, 0, 4 * sizeof(unsigned long long), s));
        mpc::AllocateFloorParams p{};
        p.profile = d_profile;
        p.counts = d_counts;
        p.floor = d_floor;
        p.must = d_must;
        p.n = n;
        p.K = c->K;
        p.lambda = mpc::budget_lambda(j);
        p.depth = d_depth;
        p.out_counts = d_out_counts;
        p.send = d_send;
        p.totals = d_totals;
        p.emphasis = d_emphasis;
        p.list = d_emphasis ? d_list : nullptr;
        p.tiles = tiles;
        std::memcpy(p.weights, weights, sizeof(uint32_t) * 3 * static_cast<size_t>(c->K));
        if (const int e = mpc::launch_budget_allocate_floor(p, s); e != 0) return launch_failed(e);
        return MPC_OK;
    });
}

}  // extern "C"

// ---- the session's budget call ----
namespace {

constexpr size_t kPatchHeader = 40;             // an empty patch; the least a call can cost

// the session's T-sized state and scratch of a budget call, carved once from d->rate (the sent map lives here from call to call)
struct RateBuffers {
    uint8_t* sent = nullptr;                    // [T]
    uint8_t* floor_t = nullptr;                 // [T] per tile
    uint8_t* must_t = nullptr;
    uint8_t* floor_c = nullptr;                 // [T] per candidate
    uint8_t* must_c = nullptr;
    uint8_t* send = nullptr;                    // [T] per candidate: the last probe's
    uint8_t* depth[2] = {nullptr, nullptr};     // [T] per candidate: the last probe's and the kept one's
    int32_t* idx[2] = {nullptr, nullptr};       // [T] the candidates sent, ascending
    int32_t* cand = nullptr;                    // [T] the candidates
    uint16_t* cut = nullptr;                    // [3T + 2] the allocation's cut counts
    int32_t* words = nullptr;                   // [4]: candidates, sent, the call's error word, tiles owed
    unsigned long long* totals = nullptr;       // [4] the allocation's, [4] the full packed frame's SSE
};

mpc_status rate_buffers(mpc_delta* d, RateBuffers* b) {
    const size_t T = static_cast<size_t>(d->tiles);
    const auto layout = [&](char* base) {
        Carve cv{base};
        b->sent = cv.take<uint8_t>(T);
        b->floor_t = cv.take<uint8_t>(T);
        b->must_t = cv.take<uint8_t>(T);
        b->floor_c = cv.take<uint8_t>(T);
        b->must_c = cv.take<uint8_t>(T);
        b->send = cv.take<uint8_t>(T);
        for (int k = 0; k < 2; ++k) b->depth[k] = cv.take<uint8_t>(T);
        for (int k = 0; k < 2; ++k) b->idx[k] = cv.take<int32_t>(T);
        b->cand = cv.take<int32_t>(T);
        b->cut = cv.take<uint16_t>(3 * T + 2);
        b->words = cv.take<int32_t>(4);
        b->totals = cv.take<unsigned long long>(5);
        return cv.at;
    };
    if (const mpc_status gs = d->rate.reserve(layout(nullptr), "rate session"); gs != MPC_OK) return gs;
    layout(d->rate.data());
    return MPC_OK;
}

// what the probes work on, sized by the call's candidates: grow-only, nothing in it outlives a call
struct RatePack {
    uint8_t* pixels = nullptr;                  // the candidates' packed frame
    uint16_t* counts = nullptr;                 // its records, uncut
    mpc_basis_choice* choices = nullptr;
    uint32_t* profile = nullptr;
    uint16_t* sent_counts = nullptr;            // a probe's packed frame of the candidates sent: its records, cut
    mpc_basis_choice* sent_choices = nullptr;
};

// padded: tiles of the candidates' frame (T where it is the whole frame); probe_padded: the most packed tiles a probe's frame can have.
// The two differ: a probe that sends k < T of T candidates packs them into 64 x ceil(k / 64) tiles, which exceeds T in T's last
// partial column
mpc_status rate_pack(mpc_delta* d, bool whole, const mpc::PackGeometry& g, long long padded, long long probe_padded, RatePack* r) {
    const size_t P = static_cast<size_t>(padded), Q = static_cast<size_t>(probe_padded), K = static_cast<size_t>(d->ctx->K);
    const auto layout = [&](char* base) {
        Carve cv{base};
        r->pixels = cv.take<uint8_t>(whole ? 0 : g.bytes);
        r->counts = cv.take<uint16_t>(whole ? 0 : 3 * P + 2);
        r->choices = cv.take<mpc_basis_choice>(whole ? 0 : 3 * P * K);
        r->profile = cv.take<uint32_t>(P * (K + 1));
        r->sent_counts = cv.take<uint16_t>(3 * Q + 2);
        r->sent_choices = cv.take<mpc_basis_choice>(3 * Q * K);
        return cv.at;
    };
    if (const mpc_status gs = d->pack_rate.reserve(layout(nullptr), "rate packed frames"); gs != MPC_OK) return gs;
    layout(d->pack_rate.data());
    return MPC_OK;
}

mpc_status make_patch(const mpc_delta* d, bool key, const int32_t* tiles, long long n, const ContainerMade& made, std::vector<uint8_t>* blob) {
    const std::string why = mpc::patch_make_error(d->width, d->height, key, tiles, n, made.bytes, made.nbytes);
    if (!why.empty()) return fail(MPC_ERR_HIP, "the patch: %s", why.c_str());
    *blob = mpc::patch_make(d->width, d->height, d->calls, key, tiles, n, made.bytes, made.nbytes);
    return MPC_OK;
}

// the fourth stage of a budget call: behind the records, everything up to the session's new sent map
mpc_status rate_finish(mpc_delta* d, const DeltaCall& call, hipStream_t s, const Tuning& tuning, const double* quant, size_t budget,
                       std::vector<uint8_t>* patch, mpc_rate_info* got) {
    mpc_context* c = d->ctx;
    const int K = c->K;
    const long long T = d->tiles;
    RateBuffers b;
    if (const mpc_status bs = rate_buffers(d, &b); bs != MPC_OK) return bs;
    HIP_TRY(hipMemsetAsync(b.words, 0, 4 * sizeof(int32_t), s));
    int* const d_error = b.words + 2;
    unsigned* const block_live = mpc::tile_diff_block_live(d->d_scratch, T);
    // 2. the candidates: a key frame's are every tile, every one of them must
    long long m = T;
    std::vector<int32_t> cand;                                  // empty: the identity
    if (!call.key) {
        uint8_t* flags = static_cast<uint8_t*>(d->d_scratch);   // the diff's, 1 = changed
        if (const int e = mpc::launch_owed_flags(b.sent, d->d_counts, T, K, flags, b.floor_t, b.must_t, s); e != 0) return launch_failed(e);
        if (const int e = mpc::launch_tile_flags_list(flags, T, block_live, b.cand, b.words, s); e != 0) return launch_failed(e);
        int32_t count = -1;
        HIP_TRY(hipMemcpyAsync(&count, b.words, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (count < 0 || count > T) return fail(MPC_ERR_HIP, "%d candidates of %lld tiles", count, T);
        m = count;
        if (m > 0 && m < T) {
            cand.resize(static_cast<size_t>(m));
            HIP_TRY(hipMemcpyAsync(cand.data(), b.cand, sizeof(int32_t) * cand.size(), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
    }
    got->candidates = static_cast<int>(m);
    got->lambda_index = -1;
    ContainerMade nothing;
    long long sent_now = 0;                                     // tiles the returned patch carries
    int kept = -1;                                              // which of depth / idx the returned patch's are; -1: every candidate at K
    if (m == 0) {
        // 3. the empty patch
        if (const mpc_status ps = make_patch(d, false, nullptr, 0, nothing, patch); ps != MPC_OK) return ps;
        got->all_bytes = patch->size();
    } else {
        // 4. the candidates' packed frame and its records; every tile a candidate: the frame and the store themselves
        const bool whole = m == T;
        const mpc::PackGeometry g = whole ? mpc::PackGeometry{0, 0, 0, 0} : mpc::pack_geometry(m, MPC_DELTA_PACK_ROWS);
        const long long padded = whole ? T : static_cast<long long>(g.rows) * g.cols;
        const int width = whole ? d->width : 8 * g.cols, height = whole ? d->height : 8 * g.rows;
        // a probe packs the k <= m candidates it sends by themselves: at most the packed frame of all m, whatever `whole` says
        const mpc::PackGeometry g_all = mpc::pack_geometry(m, MPC_DELTA_PACK_ROWS);
        const long long probe_padded = static_cast<long long>(g_all.rows) * g_all.cols;
        RatePack r;
        if (const mpc_status rs = rate_pack(d, whole, g, padded, probe_padded, &r); rs != MPC_OK) return rs;
        const uint8_t* pixels = d->d_kept;
        const uint16_t* counts = d->d_counts;
        const mpc_basis_choice* choices = d->d_choices;
        const uint8_t* floor = call.key ? nullptr : b.floor_t;
        const uint8_t* must = call.key ? nullptr : b.must_t;
        mpc::GatherParams gp{};
        gp.counts = d->d_counts;
        gp.choices = reinterpret_cast<const uint32_t*>(d->d_choices);
        gp.tiles = T;
        gp.list = b.cand;
        gp.m = m;
        gp.K = K;
        gp.error = d_error;
        if (!whole) {
            if (const int e = mpc::launch_tile_pack(d->d_kept, d->width, d->height, 3 * static_cast<size_t>(d->width), b.cand, m, g.rows, g.cols, r.pixels,
                                                    g.stride, s);
                e != 0)
                return launch_failed(e);
            mpc::GatherParams all = gp;
            all.n = m;
            all.padded = padded;
            all.out_counts = r.counts;
            all.out_choices = reinterpret_cast<uint32_t*>(r.choices);
            all.tile_bytes[0] = b.floor_t;
            all.tile_bytes[1] = b.must_t;
            all.out_bytes[0] = b.floor_c;
            all.out_bytes[1] = b.must_c;
            if (const int e = mpc::launch_gather_records(all, s); e != 0) return launch_failed(e);
            pixels = r.pixels;
            counts = r.counts;
            choices = r.choices;
            floor = b.floor_c;
            must = b.must_c;
        }
        HIP_TRY(hipMemsetAsync(b.totals + 4, 0, sizeof(unsigned long long), s));
        if (const mpc_status ds = mpc_distortion_device(c, counts, choices, quant, pixels, width, height, b.totals + 4, nullptr, s); ds != MPC_OK) return ds;
        ContainerMade full;
        if (const mpc_status fs = records_container(c, tuning, s, counts, choices, padded, width, height, quant, mpc::kIndexIntervalDefault, &full);
            fs != MPC_OK)
            return fs;
        unsigned long long full_sse = 0;
        int error_word = 0;                                     // the gather's: a candidate outside the frame
        HIP_TRY(hipMemcpyAsync(&full_sse, b.totals + 4, sizeof(full_sse), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&error_word, d_error, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (error_word) return fail(MPC_ERR_HIP, "a candidate outside the frame");
        std::vector<uint8_t> all_patch;
        if (const mpc_status ps = make_patch(d, whole, cand.data(), m, full, &all_patch); ps != MPC_OK) return ps;
        got->all_bytes = all_patch.size();
        if (all_patch.size() <= budget) {
            patch->swap(all_patch);
            sent_now = m;
            got->sse = full_sse;
        } else {
            // 5. the weights from F's index, the profile once
            uint32_t weights[3 * MPC_MAX_K];
            const int verdict = mpc::budget_weights(full.index.data(), full.index.size(), weights);
            if (verdict != 0) return fail(MPC_ERR_HIP, "the full container's seek index does not read back");
            if (const mpc_status ps = profile_on_device(c, counts, choices, quant, pixels, width, height, r.profile, d_error, s); ps != MPC_OK) return ps;
            int spare = 0;
            unsigned long long kept_totals[4] = {0, 0, 0, 0};
            size_t probed_bytes = 0;
            std::vector<int32_t> picked, listed;
            const auto probe = [&](int j, bool* fits) -> mpc_status {
                HIP_TRY(hipMemsetAsync(b.totals, 0, 4 * sizeof(unsigned long long), s));
                mpc::AllocateFloorParams ap{};
                ap.profile = r.profile;
                ap.counts = counts;
                ap.floor = floor;
                ap.must = must;
                ap.n = m;
                ap.K = K;
                ap.lambda = mpc::budget_lambda(j);
                ap.depth = b.depth[spare];
                ap.out_counts = b.cut;
                ap.send = b.send;
                ap.totals = b.totals;
                if (d->has_emphasis) {                           // candidate i is tile cand[i]; a key frame's candidates are the tiles themselves
                    ap.emphasis = reinterpret_cast<const uint8_t*>(d->emphasis.data());
                    ap.list = call.key ? nullptr : b.cand;
                    ap.tiles = T;
                }
                std::memcpy(ap.weights, weights, sizeof(uint32_t) * 3 * static_cast<size_t>(K));
                if (const int e = mpc::launch_budget_allocate_floor(ap, s); e != 0) return launch_failed(e);
                long long k = m;                                 // a key frame sends every tile
                if (!call.key) {
                    if (const int e = mpc::launch_tile_flags_list(b.send, m, block_live, b.idx[spare], b.words + 1, s); e != 0) return launch_failed(e);
                    int32_t count = -1;
                    HIP_TRY(hipMemcpyAsync(&count, b.words + 1, sizeof(int32_t), hipMemcpyDeviceToHost, s));
                    HIP_TRY(hipStreamSynchronize(s));
                    if (count < 0 || count > m) return fail(MPC_ERR_HIP, "%d of %lld candidates sent", count, m);
                    k = count;
                }
                ContainerMade made;
                std::vector<uint8_t> blob;
                if (k == 0) {
                    if (const mpc_status ps = make_patch(d, false, nullptr, 0, nothing, &blob); ps != MPC_OK) return ps;
                } else if (k == T) {                             // every tile: the whole frame's geometry, the store's records under the cut counts
                    if (const mpc_status cs = records_container(c, tuning, s, b.cut, d->d_choices, T, d->width, d->height, quant, 0, &made); cs != MPC_OK)
                        return cs;
                    if (const mpc_status ps = make_patch(d, true, nullptr, T, made, &blob); ps != MPC_OK) return ps;
                } else {                                         // the packed frame of exactly the candidates sent, cut to their depths
                    const mpc::PackGeometry gk = mpc::pack_geometry(k, MPC_DELTA_PACK_ROWS);
                    mpc::GatherParams some = gp;
                    some.idx = b.idx[spare];
                    some.depth = b.depth[spare];
                    some.n = k;
                    some.padded = static_cast<long long>(gk.rows) * gk.cols;
                    if (some.padded > probe_padded) return fail(MPC_ERR_HIP, "a probe of %lld packed tiles, room for %lld", some.padded, probe_padded);
                    some.out_counts = r.sent_counts;
                    some.out_choices = reinterpret_cast<uint32_t*>(r.sent_choices);
                    if (const int e = mpc::launch_gather_records(some, s); e != 0) return launch_failed(e);
                    if (const mpc_status cs = records_container(c, tuning, s, r.sent_counts, r.sent_choices, some.padded, 8 * gk.cols, 8 * gk.rows, quant, 0,
                                                                &made);
                        cs != MPC_OK)
                        return cs;
                    picked.resize(static_cast<size_t>(k));
                    HIP_TRY(hipMemcpyAsync(picked.data(), b.idx[spare], sizeof(int32_t) * picked.size(), hipMemcpyDeviceToHost, s));
                    HIP_TRY(hipStreamSynchronize(s));
                    listed.resize(picked.size());
                    for (size_t i = 0; i < picked.size(); ++i) {
                        if (picked[i] < 0 || picked[i] >= m) return fail(MPC_ERR_HIP, "candidate %d of %lld", picked[i], m);
                        listed[i] = cand.empty() ? picked[i] : cand[static_cast<size_t>(picked[i])];
                    }
                    if (const mpc_status ps = make_patch(d, false, listed.data(), k, made, &blob); ps != MPC_OK) return ps;
                }
                ++got->probes;
                probed_bytes = blob.size();
                *fits = blob.size() <= budget;
                if (*fits) {
                    HIP_TRY(hipMemcpyAsync(kept_totals, b.totals, sizeof(kept_totals), hipMemcpyDeviceToHost, s));
                    HIP_TRY(hipStreamSynchronize(s));
                    patch->swap(blob);
                    sent_now = k;
                    kept = spare;
                    spare ^= 1;
                }
                return MPC_OK;
            };
            // the profile kernel and the first probe's gather ran in front of the first probe's end
            const auto read_error_word = [&]() -> mpc_status {
                HIP_TRY(hipMemcpyAsync(&error_word, d_error, sizeof(int), hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                return error_word ? fail(MPC_ERR_BITSTREAM, "Invalid bitstream") : MPC_OK;
            };
            // 6. the search; its first probe, at 255: every must tile at depth 0 and nothing else
            if (const mpc_status ss = multiplier_search(probe, read_error_word, &got->lambda_index); ss != MPC_OK) return ss;
            if (got->lambda_index < 0)
                return fail(MPC_ERR_ARGUMENT, "a budget of %zu bytes: the patch with every tile that must be sent cut to nothing has %zu", budget, probed_bytes);
            got->sse = kept_totals[0];
        }
        // 7. commit: what the receiver holds once it has applied the patch
        if (kept < 0) {
            if (whole) HIP_TRY(hipMemsetAsync(b.sent, K, static_cast<size_t>(T), s));
            else if (const int e = mpc::launch_sent_commit(b.cand, m, nullptr, nullptr, m, K, b.sent, T, s); e != 0) return launch_failed(e);
        } else if (sent_now == T) {
            HIP_TRY(hipMemcpyAsync(b.sent, b.depth[kept], static_cast<size_t>(T), hipMemcpyDeviceToDevice, s));
        } else if (sent_now > 0) {
            if (const int e = mpc::launch_sent_commit(b.cand, m, b.idx[kept], b.depth[kept], sent_now, K, b.sent, T, s); e != 0) return launch_failed(e);
        }
    }
    // what is still owed: the owed-flags kernel over cleared flags and the flag count, one word back; nothing sent, nothing changed:
    // what the last call left.  The map itself stays on the device until mpc_delta_sent asks for it
    if (sent_now > 0 || call.n > 0 || !d->sent_valid) {
        uint8_t* flags = static_cast<uint8_t*>(d->d_scratch);
        HIP_TRY(hipMemsetAsync(flags, 0, static_cast<size_t>(T), s));
        if (const int e = mpc::launch_owed_flags(b.sent, d->d_counts, T, K, flags, b.floor_t, b.must_t, s); e != 0) return launch_failed(e);
        if (const int e = mpc::launch_tile_flags_list(flags, T, block_live, b.cand, b.words + 3, s); e != 0) return launch_failed(e);
        int32_t count = -1;
        HIP_TRY(hipMemcpyAsync(&count, b.words + 3, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (count < 0 || count > T) return fail(MPC_ERR_HIP, "%d of %lld tiles owed", count, T);
        d->owed = count;
    }
    d->d_sent = b.sent;
    got->owed = static_cast<int>(d->owed);
    got->sent_tiles = static_cast<int>(sent_now);
    got->key = call.key || sent_now == T ? 1 : 0;
    return MPC_OK;
}

}  // namespace

extern "C" {

mpc_status mpc_delta_encode_patch_budget(mpc_delta* d, const uint8_t* rgb, size_t row_stride, const double* quant, unsigned flags, size_t budget,
                                         uint8_t** patch, size_t* patch_bytes, mpc_rate_info* info) {
    return guarded([&]() -> mpc_status {
        if (!d || !rgb || !patch || !patch_bytes || !info) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (budget < kPatchHeader) return fail(MPC_ERR_ARGUMENT, "a budget of %zu bytes: an empty patch has %zu", budget, kPatchHeader);
        mpc_rate_info got{};
        std::vector<uint8_t> blob;
        mpc_delta_info base{};
        const mpc_status st = delta_call(
            d, rgb, row_stride, quant, flags, !d->sent_valid, &base,
            [&] {
                *patch = nullptr;
                *patch_bytes = 0;
                *info = mpc_rate_info{};
            },
            [&](const DeltaCall& call, hipStream_t s, const Tuning& tuning) -> mpc_status {
                if (const mpc_status fs = rate_finish(d, call, s, tuning, quant, budget, &blob, &got); fs != MPC_OK) return fs;
                uint8_t* out = static_cast<uint8_t*>(std::malloc(blob.size()));
                if (!out) return fail(MPC_ERR_ALLOC, "no patch");
                std::memcpy(out, blob.data(), blob.size());
                *patch = out;
                *patch_bytes = blob.size();
                d->sent_valid = true;
                return MPC_OK;
            });
        if (st != MPC_OK) return st;
        got.tiles = base.tiles;
        got.changed = base.changed;
        *info = got;
        return MPC_OK;
    });
}

mpc_status mpc_delta_sent(const mpc_delta* d, uint8_t* depth, int capacity, int* n) {
    if (!d || !n || (capacity > 0 && !depth)) return fail(MPC_ERR_ARGUMENT, "null argument");
    if (!d->sent_valid) return fail(MPC_ERR_ARGUMENT, "the session has no sent map: its last successful call was not a budget call");
    const long long count = d->tiles;
    *n = static_cast<int>(count);
    if (capacity < count) return capacity > 0 ? fail(MPC_ERR_ARGUMENT, "room for %d tiles of %lld", capacity, count) : MPC_OK;
    // the session's calls are synchronous: nothing is in flight on its stream
    if (d->ctx && d->ctx->device >= 0) HIP_TRY(hipSetDevice(d->ctx->device));
    HIP_TRY(hipMemcpy(depth, d->d_sent, static_cast<size_t>(count), hipMemcpyDeviceToHost));
    return MPC_OK;
}

}  // extern "C"

