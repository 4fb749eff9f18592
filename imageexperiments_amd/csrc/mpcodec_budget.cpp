// mpcodec_budget.cpp -- product: encode to a byte budget (include/mpcodec.h, "budget"; DESIGN.md 4, "Encoder: a byte budget").
// One pursuit, the full container with its seek index, the depth profile (mp_budget.hip), then a bisection over the multiplier
// table (multiplier_search, which the delta stream's budget call in mpcodec_rate.cpp runs too): every probe is the allocation kernel
// and one records-to-container job on the same records with the cut counts array.
// And encode to a target quality ("quality"; DESIGN.md 4, "Encoder: a target quality"): the same start (CutEncode, the front end of
// both), then the sweep kernel's totals at all 256 multipliers, the pick on the host, one allocation and one more container job.
// Both with an emphasis map ("emphasis"; DESIGN.md 4, "Encoder: emphasis"): the same bodies with a map handed to the allocation and the
// sweep, a null map being the plain call.
// And both for a group of frames of one geometry ("group"; DESIGN.md 4, "Encoder: a group of frames"): GroupEncode, the same start on n
// frames with one pursuit launch, then the same search or sweep with the group kernels, one multiplier across all tiles of all frames.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "host_budget.h"
#include "host_codec.h"
#include "mpc_internal.h"

static_assert(mpc::kBudgetLambdas == MPC_BUDGET_LAMBDAS, "one size for the multiplier table");
static_assert(mpc::kEmphasisNeutral == MPC_EMPHASIS_NEUTRAL && mpc::kEmphasisMax == MPC_EMPHASIS_MAX, "one range for the emphasis map");

namespace {

// mpc_rate_distortion's geometry
mpc_status geometry(int width, int height, long long* tiles) {
    if (width < 1 || height < 1) return fail(MPC_ERR_ARGUMENT, "bad geometry %dx%d", width, height);
    *tiles = static_cast<long long>((width + 7) / 8) * ((height + 7) / 8);
    if (*tiles * 3 >= (1LL << 31)) return fail(MPC_ERR_ARGUMENT, "frame too large");
    return MPC_OK;
}

// d_totals zeroed on `s`, then the kernel.  d_emphasis: null = the plain allocation
mpc_status allocate_on_device(const mpc_context* c, const uint32_t* d_profile, const uint16_t* d_counts, const uint8_t* d_emphasis, long long tiles,
                              const uint32_t* weights, int j, uint8_t* d_depth, uint16_t* d_out_counts, unsigned long long* d_totals, hipStream_t s) {
    HIP_TRY(hipMemsetAsync(d_totals, 0, 3 * sizeof(unsigned long long), s));
    mpc::AllocateParams p{};
    p.profile = d_profile;
    p.counts = d_counts;
    p.tiles = tiles;
    p.K = c->K;
    p.lambda = mpc::budget_lambda(j);
    p.depth = d_depth;
    p.out_counts = d_out_counts;
    p.totals = d_totals;
    p.emphasis = d_emphasis;
    std::memcpy(p.weights, weights, sizeof(uint32_t) * 3 * static_cast<size_t>(c->K));
    const int err = mpc::launch_budget_allocate(p, s);
    if (err != 0) return launch_failed(err);
    return MPC_OK;
}

// What the whole-frame cut encodes -- to a byte budget, to a target quality, each with or without an emphasis map -- start with, on
// the stack of the call.  From open() to its end it holds the context's host_calls lock, and whatever happens it leaves nothing of the
// call running.
//   arguments()      the checks that need nothing but the arguments: `tiles`
//   open()           the other refusals, the caller's outputs cleared, the staging in c->budget_dev with the frame and the map in it, one
//                    pursuit of the whole frame with the records kept, the full frame's SSE, the full container with its seek index:
//                    `full`, got.full_bytes, got.full_sse, got.full_records
//   weigh()          the rate weights from the full container's index, the depth profile once
//   cut_container()  the container of the cut counts, with the index the caller asked for
//   deliver()        a container, its index and `got` to the caller
// Info: mpc_budget_info or mpc_quality_info.  emphasis: null = every tile counts the same; else `tiles` bytes, in device memory when
// on_device, which only the allocation and the sweep read
template <class Info>
struct CutEncode {
    mpc_context* c;
    const uint8_t* rgb;
    bool on_device;
    const uint8_t* emphasis;
    int width, height;
    const double* quant;
    int index_interval;
    uint8_t** bytes;
    size_t* nbytes;
    uint8_t** index;
    size_t* index_bytes;
    Info* info;

    long long tiles = 0;
    unsigned every = 0;                                         // the index the caller gets; the full container's is made in any case: the weights come from it
    std::unique_lock<std::recursive_mutex> one_host_call;
    Tuning tuning;
    hipStream_t s = nullptr;
    Info got{};                                                 // the caller's only on success
    ContainerMade full;
    const uint8_t* frame = nullptr;                             // the frame and the map on the device
    const uint8_t* d_emphasis = nullptr;
    uint8_t* d_frame = nullptr;                                 // a host frame's copy
    uint16_t* d_counts = nullptr;
    uint16_t* d_cut = nullptr;
    mpc_basis_choice* d_choices = nullptr;
    uint32_t* d_profile = nullptr;
    uint8_t* d_depth = nullptr;
    void* d_extra = nullptr;                                    // what open()'s caller asked for
    unsigned long long* d_words = nullptr;                      // the allocation's three totals, the full frame's SSE
    int* d_error = nullptr;
    uint8_t* d_map = nullptr;                                   // a host emphasis map's copy

    ~CutEncode() {
        if (s) (void)hipStreamSynchronize(s);
    }

    mpc_status arguments() {
        if (!c || !rgb || !bytes || !nbytes || !info) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (index_interval >= 0 && (!index || !index_bytes)) return fail(MPC_ERR_ARGUMENT, "null argument");
        return geometry(width, height, &tiles);
    }

    size_t layout(char* base, size_t extra_bytes) {
        const size_t n_tc = 3 * static_cast<size_t>(tiles), K = static_cast<size_t>(c->K);
        Carve cv{base};
        d_frame = cv.take<uint8_t>(on_device ? 0 : 3 * static_cast<size_t>(width) * static_cast<size_t>(height));
        d_counts = cv.take<uint16_t>(n_tc + 2);
        d_cut = cv.take<uint16_t>(n_tc + 2);
        d_choices = cv.take<mpc_basis_choice>(n_tc * K);
        d_profile = cv.take<uint32_t>(static_cast<size_t>(tiles) * (K + 1));
        d_depth = cv.take<uint8_t>(static_cast<size_t>(tiles));
        d_extra = cv.take<char>(extra_bytes);
        d_words = cv.take<unsigned long long>(4);
        d_error = cv.take<int>(1);
        d_map = cv.take<uint8_t>(emphasis && !on_device ? static_cast<size_t>(tiles) : 0);
        return cv.at;
    }

    // extra_bytes: device memory of the caller's own, behind the depth map (d_extra)
    mpc_status open(size_t extra_bytes) {
        if (const mpc_status bad = optional_index_interval_of(index_interval, &every)) return bad;
        if (c->device < 0) return no_device();
        one_host_call = std::unique_lock<std::recursive_mutex>(c->host_calls);
        for (int k = 0; k < mpc_context::kSeqSlots; ++k)
            if (c->jobs[k] && c->jobs[k]->stage != 0) return fail(MPC_ERR_ARGUMENT, "container job slot %d is busy", k);
        *bytes = nullptr;
        *nbytes = 0;
        if (index) *index = nullptr;
        if (index_bytes) *index_bytes = 0;
        *info = Info{};
        HIP_TRY(hipSetDevice(c->device));
        tuning = read_tuning();
        if (!c->budget_stream) HIP_TRY(hipStreamCreateWithFlags(&c->budget_stream, hipStreamNonBlocking));
        s = c->budget_stream;
        if (const mpc_status gs = c->budget_dev.reserve(layout(nullptr, extra_bytes), "budget staging"); gs != MPC_OK) return gs;
        layout(c->budget_dev.data(), extra_bytes);
        const size_t row = 3 * static_cast<size_t>(width);
        frame = rgb;
        if (!on_device) {
            HIP_TRY(hipMemcpyAsync(d_frame, rgb, row * static_cast<size_t>(height), hipMemcpyHostToDevice, s));
            frame = d_frame;
        }
        d_emphasis = emphasis;
        if (emphasis && !on_device) {
            HIP_TRY(hipMemcpyAsync(d_map, emphasis, static_cast<size_t>(tiles), hipMemcpyHostToDevice, s));
            d_emphasis = d_map;
        }
        HIP_TRY(hipMemsetAsync(d_words, 0, 4 * sizeof(unsigned long long), s));
        HIP_TRY(hipMemsetAsync(d_error, 0, sizeof(int), s));
        // one pursuit of the whole frame, the records kept; the full frame's SSE behind it
        if (const mpc_status es = mpc_encode_tiles_device(c, frame, width, height, row, 0, (height + 7) / 8, quant, d_counts, d_choices, nullptr, nullptr, 0, s);
            es != MPC_OK)
            return es;
        if (const mpc_status ds = mpc_distortion_device(c, d_counts, d_choices, quant, frame, width, height, d_words + 3, nullptr, s); ds != MPC_OK)
            return ds;
        // the full container with its seek index; the job returns with `s` drained
        if (const mpc_status fs = records_container(c, tuning, s, d_counts, d_choices, tiles, width, height, quant, every ? every : mpc::kIndexIntervalDefault, &full);
            fs != MPC_OK)
            return fs;
        HIP_TRY(hipMemcpyAsync(&got.full_sse, d_words + 3, sizeof(got.full_sse), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const size_t K = static_cast<size_t>(c->K);
        mpc::ContainerIndex full_index;
        if (!mpc::read_container_index(full.index.data(), full.index.size(), full_index) || full_index.streams.size() != 1 + 6 * K)
            return fail(MPC_ERR_HIP, "the full container's seek index does not read back");
        for (size_t ch = 0; ch < 3; ++ch)
            for (size_t i = 0; i < K; ++i) got.full_records += full_index.streams[1 + 2 * K * ch + 2 * i].expect;
        got.full_bytes = full.nbytes;
        return MPC_OK;
    }

    mpc_status weigh(uint32_t* weights) {
        const int verdict = mpc::budget_weights(full.index.data(), full.index.size(), weights);
        if (verdict == 2) return fail(MPC_ERR_ARGUMENT, "the full container's seek index is serial only: no stream sizes to weigh the steps with");
        if (verdict != 0) return fail(MPC_ERR_HIP, "the full container's seek index does not read back");
        return profile_on_device(c, d_counts, d_choices, quant, frame, width, height, d_profile, d_error, s);
    }

    mpc_status cut_container(ContainerMade* made) {
        return records_container(c, tuning, s, d_cut, d_choices, tiles, width, height, quant, every, made);
    }

    mpc_status deliver(ContainerMade& made) {
        if (const mpc_status ds = deliver_container(made, every, bytes, nbytes, index, index_bytes); ds != MPC_OK) return ds;
        *info = got;
        return MPC_OK;
    }
};

// d_totals[768] zeroed on `s`, then the kernel.  d_emphasis: null = the plain sweep
mpc_status sweep_on_device(const mpc_context* c, const uint32_t* d_profile, const uint16_t* d_counts, const uint8_t* d_emphasis, long long tiles,
                           const uint32_t* weights, unsigned long long* d_totals, hipStream_t s) {
    HIP_TRY(hipMemsetAsync(d_totals, 0, 3 * mpc::kBudgetLambdas * sizeof(unsigned long long), s));
    mpc::SweepParams p{};
    p.profile = d_profile;
    p.counts = d_counts;
    p.tiles = tiles;
    p.K = c->K;
    p.totals = d_totals;
    p.emphasis = d_emphasis;
    std::memcpy(p.weights, weights, sizeof(uint32_t) * 3 * static_cast<size_t>(c->K));
    const int err = mpc::launch_budget_sweep(p, s);
    if (err != 0) return launch_failed(err);
    return MPC_OK;
}

// mpc_encode_image_budget: the full container if it fits, else the search over the multiplier table, every probe the allocation and the
// container of its cut counts
mpc_status encode_budget(mpc_context* c, const uint8_t* rgb, bool on_device, const uint8_t* emphasis, int width, int height, const double* quant,
                         size_t budget, int index_interval, uint8_t** bytes, size_t* nbytes, uint8_t** index, size_t* index_bytes, uint8_t* depth,
                         mpc_budget_info* info) {
    return guarded([&]() -> mpc_status {
        CutEncode<mpc_budget_info> e{c, rgb, on_device, emphasis, width, height, quant, index_interval, bytes, nbytes, index, index_bytes, info};
        if (const mpc_status as = e.arguments(); as != MPC_OK) return as;
        if (budget == 0) return fail(MPC_ERR_ARGUMENT, "a budget of 0 bytes");
        if (const mpc_status os = e.open(static_cast<size_t>(e.tiles)); os != MPC_OK) return os;      // a second depth map
        uint8_t* const d_depth[2] = {e.d_depth, static_cast<uint8_t*>(e.d_extra)};
        mpc_budget_info& got = e.got;
        hipStream_t s = e.s;
        ContainerMade best;
        int best_depth = -1;                                        // which of d_depth holds the returned container's map; -1: no cut
        if (e.full.nbytes <= budget) {
            best.swap(e.full);
            got.lambda_index = -1;
            got.probes = 0;
            got.sse = got.full_sse;
            got.records = got.full_records;
        } else {
            uint32_t weights[3 * MPC_MAX_K];
            if (const mpc_status ws = e.weigh(weights); ws != MPC_OK) return ws;
            int spare = 0;
            unsigned long long best_totals[3] = {0, 0, 0};
            size_t probed_bytes = 0;                                // the last probe's size
            // size(j): the container of the cut counts at j; kept when it fits
            const auto probe = [&](int j, bool* fits) -> mpc_status {
                if (const mpc_status as = allocate_on_device(c, e.d_profile, e.d_counts, e.d_emphasis, e.tiles, weights, j, d_depth[spare], e.d_cut, e.d_words, s);
                    as != MPC_OK)
                    return as;
                ContainerMade made;
                if (const mpc_status cs = e.cut_container(&made); cs != MPC_OK) return cs;
                ++got.probes;
                probed_bytes = made.nbytes;
                *fits = made.nbytes <= budget;
                if (*fits) {
                    HIP_TRY(hipMemcpyAsync(best_totals, e.d_words, sizeof(best_totals), hipMemcpyDeviceToHost, s));
                    HIP_TRY(hipStreamSynchronize(s));
                    best.swap(made);
                    best_depth = spare;
                    spare ^= 1;
                }
                return MPC_OK;
            };
            const auto read_error_word = [&]() -> mpc_status {      // the profile kernel ran in front of the first probe
                int error_word = 0;
                HIP_TRY(hipMemcpyAsync(&error_word, e.d_error, sizeof(int), hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                return error_word ? fail(MPC_ERR_BITSTREAM, "Invalid bitstream") : MPC_OK;
            };
            if (const mpc_status ss = multiplier_search(probe, read_error_word, &got.lambda_index); ss != MPC_OK) return ss;
            if (got.lambda_index < 0)                               // the smallest container there is
                return fail(MPC_ERR_ARGUMENT, "a budget of %zu bytes: the container with every tile cut to nothing has %zu", budget, probed_bytes);
            got.sse = best_totals[0];
            got.records = best_totals[2];
        }
        // the container kept from the search's last probe that fitted, and its depth map
        if (depth) {
            if (best_depth < 0) std::memset(depth, c->K, static_cast<size_t>(e.tiles));
            else {
                HIP_TRY(hipMemcpyAsync(depth, d_depth[best_depth], static_cast<size_t>(e.tiles), hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
            }
        }
        return e.deliver(best);
    });
}

// mpc_encode_image_quality: the sweep's totals at all 256 multipliers, the pick on the host, one allocation and its container
mpc_status encode_quality(mpc_context* c, const uint8_t* rgb, bool on_device, const uint8_t* emphasis, int width, int height, const double* quant,
                          unsigned long long max_sse, int index_interval, uint8_t** bytes, size_t* nbytes, uint8_t** index, size_t* index_bytes, uint8_t* depth,
                          mpc_quality_info* info) {
    return guarded([&]() -> mpc_status {
        std::vector<unsigned long long> totals(3 * mpc::kBudgetLambdas);     // in front of `e`: it outlives the drain
        CutEncode<mpc_quality_info> e{c, rgb, on_device, emphasis, width, height, quant, index_interval, bytes, nbytes, index, index_bytes, info};
        if (const mpc_status as = e.arguments(); as != MPC_OK) return as;
        if (const mpc_status os = e.open(totals.size() * sizeof(unsigned long long)); os != MPC_OK) return os;   // the sweep's 768 totals
        unsigned long long* const d_sweep = static_cast<unsigned long long*>(e.d_extra);
        mpc_quality_info& got = e.got;
        hipStream_t s = e.s;
        uint32_t weights[3 * MPC_MAX_K];
        if (const mpc_status ws = e.weigh(weights); ws != MPC_OK) return ws;
        // the sweep: one launch for all 256 multipliers, its totals to the host
        if (const mpc_status ss = sweep_on_device(c, e.d_profile, e.d_counts, e.d_emphasis, e.tiles, weights, d_sweep, s); ss != MPC_OK) return ss;
        int error_word = 0;
        HIP_TRY(hipMemcpyAsync(totals.data(), d_sweep, totals.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&error_word, e.d_error, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (error_word) return fail(MPC_ERR_BITSTREAM, "Invalid bitstream");
        got.min_sse = totals[0];
        // the largest multiplier whose distortion is within the target
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the totals are u64");
        const int j = mpc::quality_pick(reinterpret_cast<const uint64_t*>(totals.data()), max_sse);
        // no cut is that good
        if (j < 0)
            return fail(MPC_ERR_ARGUMENT, "a squared error of at most %llu: the best that cutting this frame's records reaches is %llu", max_sse, totals[0]);
        // the allocation at j and its container, the index with it if asked for
        if (const mpc_status as = allocate_on_device(c, e.d_profile, e.d_counts, e.d_emphasis, e.tiles, weights, j, e.d_depth, e.d_cut, e.d_words, s); as != MPC_OK)
            return as;
        ContainerMade made;
        if (const mpc_status cs = e.cut_container(&made); cs != MPC_OK) return cs;
        unsigned long long at_j[3] = {0, 0, 0};
        HIP_TRY(hipMemcpyAsync(at_j, e.d_words, sizeof(at_j), hipMemcpyDeviceToHost, s));
        if (depth) HIP_TRY(hipMemcpyAsync(depth, e.d_depth, static_cast<size_t>(e.tiles), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (std::memcmp(at_j, totals.data() + 3 * static_cast<size_t>(j), sizeof(at_j)) != 0)
            return fail(MPC_ERR_HIP, "the allocation at multiplier %d does not give the sweep's totals", j);
        got.lambda_index = j;
        got.sse = at_j[0];
        got.model_bits_256 = at_j[1];
        got.records = at_j[2];
        return e.deliver(made);
    });
}

// ---- a group of frames (include/mpcodec.h, "group"; DESIGN.md 4, "Encoder: a group of frames") ----
static_assert(mpc::kGroupMaxFrames == MPC_GROUP_MAX_FRAMES, "one limit for the frames of a group");

// d_totals[frames][3] zeroed on `s`, then the kernel, a launch per mpc::kGroupChunk frames.  d_emphasis: null = the plain allocation
mpc_status allocate_group_on_device(const mpc_context* c, const uint32_t* d_profile, const uint16_t* d_counts, const uint8_t* d_emphasis, int frames,
                                    long long tiles, const uint32_t* weights, int j, uint8_t* d_depth, uint16_t* d_out_counts,
                                    unsigned long long* d_totals, hipStream_t s) {
    HIP_TRY(hipMemsetAsync(d_totals, 0, 3 * static_cast<size_t>(frames) * sizeof(unsigned long long), s));
    const int err = mpc::launch_budget_allocate_group(d_profile, d_counts, d_emphasis, frames, tiles, c->K, weights, mpc::budget_lambda(j), d_depth,
                                                      d_out_counts, d_totals, s);
    if (err != 0) return launch_failed(err);
    return MPC_OK;
}

// d_totals[768] zeroed on `s`, then the kernel, a launch per mpc::kGroupChunk frames
mpc_status sweep_group_on_device(const mpc_context* c, const uint32_t* d_profile, const uint16_t* d_counts, const uint8_t* d_emphasis, int frames,
                                 long long tiles, const uint32_t* weights, unsigned long long* d_totals, hipStream_t s) {
    HIP_TRY(hipMemsetAsync(d_totals, 0, 3 * mpc::kBudgetLambdas * sizeof(unsigned long long), s));
    const int err = mpc::launch_budget_sweep_group(d_profile, d_counts, d_emphasis, frames, tiles, c->K, weights, d_totals, s);
    if (err != 0) return launch_failed(err);
    return MPC_OK;
}

// what the device pieces of a group refuse before anything is enqueued
mpc_status group_arguments(int frames, long long tiles) {
    if (frames < 1 || frames > MPC_GROUP_MAX_FRAMES) return fail(MPC_ERR_ARGUMENT, "%d frames: 1 to %d", frames, MPC_GROUP_MAX_FRAMES);
    if (tiles < 1 || tiles * 3 * frames >= (1LL << 31)) return fail(MPC_ERR_ARGUMENT, "%d frames of %lld tiles", frames, tiles);
    return MPC_OK;
}

void add_to(mpc_budget_info& sum, const mpc_budget_info& one) {
    sum.lambda_index = one.lambda_index;
    sum.probes = one.probes;
    sum.full_bytes += one.full_bytes;
    sum.sse += one.sse;
    sum.full_sse += one.full_sse;
    sum.records += one.records;
    sum.full_records += one.full_records;
}

void add_to(mpc_quality_info& sum, const mpc_quality_info& one) {
    sum.lambda_index = one.lambda_index;
    sum.full_bytes += one.full_bytes;
    sum.sse += one.sse;
    sum.full_sse += one.full_sse;
    sum.min_sse += one.min_sse;
    sum.records += one.records;
    sum.full_records += one.full_records;
    sum.model_bits_256 += one.model_bits_256;
}

// CutEncode for `n` frames of one geometry: what the group's budget and quality encodes start with.  The same steps in the same order --
// with n = 1 the same launches and jobs on the same records, so the same bytes -- with one pursuit of the whole group
// (mpc_encode_batch_device on the frames side by side in the staging: device frames are copied there too, a batch launch takes a stride),
// and everything per tile frame-major: frame f's records, profile, depth and cut counts at tile f * tiles.
//   arguments()      `tiles` of one frame
//   open()           full[f], got[f].full_bytes, .full_sse, .full_records
//   weigh()          weights[f][3K] from full[f]'s index, frame f's depth profile
//   cut_container()  frame f's container of the cut counts
//   deliver()        the containers, their indexes, got[f] and the sums
template <class Info>
struct GroupEncode {
    mpc_context* c;
    const uint8_t* const* frames;
    bool on_device;
    const uint8_t* emphasis;
    int n, width, height;
    const double* quant;
    int index_interval;
    uint8_t** bytes;
    size_t* nbytes;
    uint8_t** indexes;
    size_t* index_bytes;
    Info* frame_info;
    Info* info;

    long long tiles = 0;
    unsigned every = 0;
    std::unique_lock<std::recursive_mutex> one_host_call;
    Tuning tuning;
    hipStream_t s = nullptr;
    std::vector<Info> got;                                      // the caller's only on success
    std::vector<ContainerMade> full;
    size_t n_tc = 0, frame_bytes = 0;
    const uint8_t* d_emphasis = nullptr;
    uint8_t* d_frames = nullptr;                                // the frames side by side
    uint16_t* d_counts = nullptr;
    uint16_t* d_cut = nullptr;
    mpc_basis_choice* d_choices = nullptr;
    uint32_t* d_profile = nullptr;
    uint8_t* d_depth = nullptr;
    void* d_extra = nullptr;
    unsigned long long* d_words = nullptr;                      // the allocation's 3n totals, then the full frames' n SSEs
    int* d_error = nullptr;
    uint8_t* d_map = nullptr;

    ~GroupEncode() {
        if (s) (void)hipStreamSynchronize(s);
    }

    mpc_status arguments() {
        if (!c || !frames || !bytes || !nbytes || !frame_info || !info) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (index_interval >= 0 && (!indexes || !index_bytes)) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (n < 1 || n > MPC_GROUP_MAX_FRAMES) return fail(MPC_ERR_ARGUMENT, "%d frames: 1 to %d", n, MPC_GROUP_MAX_FRAMES);
        for (int f = 0; f < n; ++f)
            if (!frames[f]) return fail(MPC_ERR_ARGUMENT, "frame %d is null", f);
        if (const mpc_status gs = geometry(width, height, &tiles); gs != MPC_OK) return gs;
        if (tiles * 3 * n >= (1LL << 31)) return fail(MPC_ERR_ARGUMENT, "group too large");
        n_tc = 3 * static_cast<size_t>(tiles);
        frame_bytes = 3 * static_cast<size_t>(width) * static_cast<size_t>(height);
        return MPC_OK;
    }

    const uint16_t* counts_of(int f) const { return d_counts + static_cast<size_t>(f) * n_tc; }
    const mpc_basis_choice* choices_of(int f) const { return d_choices + static_cast<size_t>(f) * n_tc * static_cast<size_t>(c->K); }
    const uint8_t* frame_of(int f) const { return d_frames + static_cast<size_t>(f) * frame_bytes; }

    size_t layout(char* base, size_t extra_bytes) {
        const size_t N = static_cast<size_t>(n), K = static_cast<size_t>(c->K), T = static_cast<size_t>(tiles);
        Carve cv{base};
        d_frames = cv.take<uint8_t>(N * frame_bytes);
        d_counts = cv.take<uint16_t>(N * n_tc + 2);
        d_cut = cv.take<uint16_t>(N * n_tc + 2);
        d_choices = cv.take<mpc_basis_choice>(N * n_tc * K);
        d_profile = cv.take<uint32_t>(N * T * (K + 1));
        d_depth = cv.take<uint8_t>(N * T);
        d_extra = cv.take<char>(extra_bytes);
        d_words = cv.take<unsigned long long>(4 * N);
        d_error = cv.take<int>(1);
        d_map = cv.take<uint8_t>(emphasis && !on_device ? N * T : 0);
        return cv.at;
    }

    mpc_status open(size_t extra_bytes) {
        if (const mpc_status bad = optional_index_interval_of(index_interval, &every)) return bad;
        if (c->device < 0) return no_device();
        one_host_call = std::unique_lock<std::recursive_mutex>(c->host_calls);
        for (int k = 0; k < mpc_context::kSeqSlots; ++k)
            if (c->jobs[k] && c->jobs[k]->stage != 0) return fail(MPC_ERR_ARGUMENT, "container job slot %d is busy", k);
        for (int f = 0; f < n; ++f) {
            bytes[f] = nullptr;
            nbytes[f] = 0;
            if (indexes) indexes[f] = nullptr;
            if (index_bytes) index_bytes[f] = 0;
            frame_info[f] = Info{};
        }
        *info = Info{};
        got.assign(static_cast<size_t>(n), Info{});
        full = std::vector<ContainerMade>(static_cast<size_t>(n));
        HIP_TRY(hipSetDevice(c->device));
        tuning = read_tuning();
        if (!c->budget_stream) HIP_TRY(hipStreamCreateWithFlags(&c->budget_stream, hipStreamNonBlocking));
        s = c->budget_stream;
        if (const mpc_status gs = c->budget_dev.reserve(layout(nullptr, extra_bytes), "budget staging"); gs != MPC_OK) return gs;
        layout(c->budget_dev.data(), extra_bytes);
        const size_t row = 3 * static_cast<size_t>(width), N = static_cast<size_t>(n);
        for (int f = 0; f < n; ++f)
            HIP_TRY(hipMemcpyAsync(d_frames + static_cast<size_t>(f) * frame_bytes, frames[f], frame_bytes,
                                   on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        d_emphasis = emphasis;
        if (emphasis && !on_device) {
            HIP_TRY(hipMemcpyAsync(d_map, emphasis, N * static_cast<size_t>(tiles), hipMemcpyHostToDevice, s));
            d_emphasis = d_map;
        }
        HIP_TRY(hipMemsetAsync(d_words, 0, 4 * N * sizeof(unsigned long long), s));
        HIP_TRY(hipMemsetAsync(d_error, 0, sizeof(int), s));
        // one pursuit of the whole group, the records kept; every full frame's SSE behind it
        if (const mpc_status es = mpc_encode_batch_device(c, d_frames, n, frame_bytes, width, height, row, 0, (height + 7) / 8, quant, d_counts, d_choices,
                                                          nullptr, nullptr, 0, s);
            es != MPC_OK)
            return es;
        unsigned long long* const d_sse = d_words + 3 * N;
        for (int f = 0; f < n; ++f)
            if (const mpc_status ds = mpc_distortion_device(c, counts_of(f), choices_of(f), quant, frame_of(f), width, height, d_sse + f, nullptr, s);
                ds != MPC_OK)
                return ds;
        // every frame's full container with its seek index; a job returns with `s` drained
        for (int f = 0; f < n; ++f)
            if (const mpc_status fs = records_container(c, tuning, s, counts_of(f), choices_of(f), tiles, width, height, quant,
                                                        every ? every : mpc::kIndexIntervalDefault, &full[static_cast<size_t>(f)]);
                fs != MPC_OK)
                return fs;
        std::vector<unsigned long long> sse(N);
        HIP_TRY(hipMemcpyAsync(sse.data(), d_sse, N * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const size_t K = static_cast<size_t>(c->K);
        for (size_t f = 0; f < N; ++f) {
            mpc::ContainerIndex full_index;
            if (!mpc::read_container_index(full[f].index.data(), full[f].index.size(), full_index) || full_index.streams.size() != 1 + 6 * K)
                return fail(MPC_ERR_HIP, "the full container's seek index does not read back");
            for (size_t ch = 0; ch < 3; ++ch)
                for (size_t i = 0; i < K; ++i) got[f].full_records += full_index.streams[1 + 2 * K * ch + 2 * i].expect;
            got[f].full_bytes = full[f].nbytes;
            got[f].full_sse = sse[f];
        }
        return MPC_OK;
    }

    size_t full_bytes() const {
        size_t sum = 0;
        for (const ContainerMade& m : full) sum += m.nbytes;
        return sum;
    }

    // weights: [n][3K]
    mpc_status weigh(uint32_t* weights) {
        for (int f = 0; f < n; ++f) {
            const ContainerMade& m = full[static_cast<size_t>(f)];
            const int verdict = mpc::budget_weights(m.index.data(), m.index.size(), weights + static_cast<size_t>(f) * 3 * static_cast<size_t>(c->K));
            if (verdict == 2) return fail(MPC_ERR_ARGUMENT, "the full container's seek index is serial only: no stream sizes to weigh the steps with");
            if (verdict != 0) return fail(MPC_ERR_HIP, "the full container's seek index does not read back");
        }
        for (int f = 0; f < n; ++f)
            if (const mpc_status ps = profile_on_device(c, counts_of(f), choices_of(f), quant, frame_of(f), width, height,
                                                        d_profile + static_cast<size_t>(f) * static_cast<size_t>(tiles) * static_cast<size_t>(c->K + 1), d_error, s);
                ps != MPC_OK)
                return ps;
        return MPC_OK;
    }

    mpc_status cut_container(int f, ContainerMade* made) {
        return records_container(c, tuning, s, d_cut + static_cast<size_t>(f) * n_tc, choices_of(f), tiles, width, height, quant, every, made);
    }

    // the frames' containers of the cut counts, one job behind the other; *sum: their bytes.  Once the sum is above `stop_above` the
    // frames behind are not made: a probe that does not fit is known as such from the frames so far
    mpc_status cut_containers(std::vector<ContainerMade>& made, size_t* sum, size_t stop_above = ~size_t{0}) {
        *sum = 0;
        for (int f = 0; f < n && *sum <= stop_above; ++f) {
            if (const mpc_status cs = cut_container(f, &made[static_cast<size_t>(f)]); cs != MPC_OK) return cs;
            *sum += made[static_cast<size_t>(f)].nbytes;
        }
        return MPC_OK;
    }

    mpc_status deliver(std::vector<ContainerMade>& made) {
        for (int f = 0; f < n; ++f) {
            const mpc_status ds = deliver_container(made[static_cast<size_t>(f)], every, bytes + f, nbytes + f, indexes ? indexes + f : nullptr,
                                                    index_bytes ? index_bytes + f : nullptr);
            if (ds != MPC_OK) {                                 // nothing is returned
                for (int k = 0; k <= f; ++k) {
                    std::free(bytes[k]);
                    bytes[k] = nullptr;
                    nbytes[k] = 0;
                    if (every) {
                        std::free(indexes[k]);
                        indexes[k] = nullptr;
                        index_bytes[k] = 0;
                    }
                }
                return ds;
            }
        }
        Info sum{};
        for (int f = 0; f < n; ++f) {
            frame_info[f] = got[static_cast<size_t>(f)];
            add_to(sum, got[static_cast<size_t>(f)]);
        }
        *info = sum;
        return MPC_OK;
    }
};

// mpc_encode_images_budget: encode_budget over the group -- the full containers if their sum fits, else the search over the multiplier
// table with size(j) the sum of the frames' containers of the group allocation's cut counts at j
mpc_status encode_group_budget(mpc_context* c, const uint8_t* const* frames, bool on_device, const uint8_t* emphasis, int n, int width, int height,
                               const double* quant, size_t budget, int index_interval, uint8_t** bytes, size_t* nbytes, uint8_t** indexes,
                               size_t* index_bytes, uint8_t* depth, mpc_budget_info* frame_info, mpc_budget_info* info) {
    return guarded([&]() -> mpc_status {
        GroupEncode<mpc_budget_info> e{c, frames, on_device, emphasis, n, width, height, quant, index_interval, bytes, nbytes, indexes, index_bytes, frame_info, info};
        if (const mpc_status as = e.arguments(); as != MPC_OK) return as;
        if (budget == 0) return fail(MPC_ERR_ARGUMENT, "a budget of 0 bytes");
        const size_t N = static_cast<size_t>(n), T = static_cast<size_t>(e.tiles);
        if (const mpc_status os = e.open(N * T); os != MPC_OK) return os;                             // a second depth map
        uint8_t* const d_depth[2] = {e.d_depth, static_cast<uint8_t*>(e.d_extra)};
        hipStream_t s = e.s;
        std::vector<ContainerMade> best(N);
        int best_depth = -1;                                        // which of d_depth holds the returned containers' map; -1: no cut
        int found = -1, probes = 0;
        if (e.full_bytes() <= budget) {
            best.swap(e.full);
            for (mpc_budget_info& g : e.got) {
                g.sse = g.full_sse;
                g.records = g.full_records;
            }
        } else {
            std::vector<uint32_t> weights(N * 3 * MPC_MAX_K);
            if (const mpc_status ws = e.weigh(weights.data()); ws != MPC_OK) return ws;
            int spare = 0;
            std::vector<unsigned long long> best_totals(3 * N, 0);
            size_t probed_bytes = 0;                                // the last probe's size
            const auto probe = [&](int j, bool* fits) -> mpc_status {
                if (const mpc_status as = allocate_group_on_device(c, e.d_profile, e.d_counts, e.d_emphasis, n, e.tiles, weights.data(), j, d_depth[spare],
                                                                   e.d_cut, e.d_words, s);
                    as != MPC_OK)
                    return as;
                std::vector<ContainerMade> made(N);
                // the last multiplier's size is made whole: the refusal names it
                if (const mpc_status cs = e.cut_containers(made, &probed_bytes, j == mpc::kBudgetLambdas - 1 ? ~size_t{0} : budget); cs != MPC_OK) return cs;
                ++probes;
                *fits = probed_bytes <= budget;
                if (*fits) {
                    HIP_TRY(hipMemcpyAsync(best_totals.data(), e.d_words, 3 * N * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
                    HIP_TRY(hipStreamSynchronize(s));
                    best.swap(made);
                    best_depth = spare;
                    spare ^= 1;
                }
                return MPC_OK;
            };
            const auto read_error_word = [&]() -> mpc_status {      // the profile kernels ran in front of the first probe
                int error_word = 0;
                HIP_TRY(hipMemcpyAsync(&error_word, e.d_error, sizeof(int), hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                return error_word ? fail(MPC_ERR_BITSTREAM, "Invalid bitstream") : MPC_OK;
            };
            if (const mpc_status ss = multiplier_search(probe, read_error_word, &found); ss != MPC_OK) return ss;
            if (found < 0)                                          // the smallest containers there are
                return fail(MPC_ERR_ARGUMENT, "a budget of %zu bytes: the containers with every tile cut to nothing have %zu", budget, probed_bytes);
            for (size_t f = 0; f < N; ++f) {
                e.got[f].sse = best_totals[3 * f];
                e.got[f].records = best_totals[3 * f + 2];
            }
        }
        for (mpc_budget_info& g : e.got) {
            g.lambda_index = found;
            g.probes = probes;
        }
        if (depth) {
            if (best_depth < 0) std::memset(depth, c->K, N * T);
            else {
                HIP_TRY(hipMemcpyAsync(depth, d_depth[best_depth], N * T, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
            }
        }
        return e.deliver(best);
    });
}

// mpc_encode_images_quality: encode_quality over the group -- the group sweep's totals, the pick, one group allocation, n container jobs
mpc_status encode_group_quality(mpc_context* c, const uint8_t* const* frames, bool on_device, const uint8_t* emphasis, int n, int width, int height,
                                const double* quant, unsigned long long max_sse, int index_interval, uint8_t** bytes, size_t* nbytes,
                                uint8_t** indexes, size_t* index_bytes, uint8_t* depth, mpc_quality_info* frame_info, mpc_quality_info* info) {
    return guarded([&]() -> mpc_status {
        std::vector<unsigned long long> totals(3 * mpc::kBudgetLambdas);     // in front of `e`: they outlive the drain
        std::vector<unsigned long long> at_0, at_j;
        GroupEncode<mpc_quality_info> e{c, frames, on_device, emphasis, n, width, height, quant, index_interval, bytes, nbytes, indexes, index_bytes, frame_info, info};
        if (const mpc_status as = e.arguments(); as != MPC_OK) return as;
        const size_t N = static_cast<size_t>(n), T = static_cast<size_t>(e.tiles);
        at_0.assign(3 * N, 0);
        at_j.assign(3 * N, 0);
        if (const mpc_status os = e.open(totals.size() * sizeof(unsigned long long)); os != MPC_OK) return os;   // the sweep's 768 totals
        unsigned long long* const d_sweep = static_cast<unsigned long long*>(e.d_extra);
        hipStream_t s = e.s;
        std::vector<uint32_t> weights(N * 3 * MPC_MAX_K);
        if (const mpc_status ws = e.weigh(weights.data()); ws != MPC_OK) return ws;
        // the sweep: one launch for all 256 multipliers and all frames; and, the sweep's totals being the group's, the allocation at
        // multiplier 0 for every frame's own least squared error
        if (const mpc_status ss = sweep_group_on_device(c, e.d_profile, e.d_counts, e.d_emphasis, n, e.tiles, weights.data(), d_sweep, s); ss != MPC_OK) return ss;
        if (const mpc_status as = allocate_group_on_device(c, e.d_profile, e.d_counts, e.d_emphasis, n, e.tiles, weights.data(), 0, e.d_depth, e.d_cut, e.d_words, s);
            as != MPC_OK)
            return as;
        int error_word = 0;
        HIP_TRY(hipMemcpyAsync(totals.data(), d_sweep, totals.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(at_0.data(), e.d_words, 3 * N * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&error_word, e.d_error, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (error_word) return fail(MPC_ERR_BITSTREAM, "Invalid bitstream");
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the totals are u64");
        const int j = mpc::quality_pick(reinterpret_cast<const uint64_t*>(totals.data()), max_sse);
        if (j < 0)
            return fail(MPC_ERR_ARGUMENT, "a squared error of at most %llu: the best that cutting these frames' records reaches is %llu", max_sse, totals[0]);
        if (const mpc_status as = allocate_group_on_device(c, e.d_profile, e.d_counts, e.d_emphasis, n, e.tiles, weights.data(), j, e.d_depth, e.d_cut, e.d_words, s);
            as != MPC_OK)
            return as;
        std::vector<ContainerMade> made(N);
        size_t made_bytes = 0;
        if (const mpc_status cs = e.cut_containers(made, &made_bytes); cs != MPC_OK) return cs;
        HIP_TRY(hipMemcpyAsync(at_j.data(), e.d_words, 3 * N * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        if (depth) HIP_TRY(hipMemcpyAsync(depth, e.d_depth, N * T, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        // the cross-check: the frames' totals at j add up to the sweep's, and those at 0 to its first
        unsigned long long sum_j[3] = {0, 0, 0}, least = 0;
        for (size_t f = 0; f < N; ++f) {
            for (int k = 0; k < 3; ++k) sum_j[k] += at_j[3 * f + static_cast<size_t>(k)];
            least += at_0[3 * f];
        }
        if (std::memcmp(sum_j, totals.data() + 3 * static_cast<size_t>(j), sizeof(sum_j)) != 0 || least != totals[0])
            return fail(MPC_ERR_HIP, "the allocation at multiplier %d does not give the sweep's totals", j);
        for (size_t f = 0; f < N; ++f) {
            mpc_quality_info& g = e.got[f];
            g.lambda_index = j;
            g.min_sse = at_0[3 * f];
            g.sse = at_j[3 * f];
            g.model_bits_256 = at_j[3 * f + 1];
            g.records = at_j[3 * f + 2];
        }
        return e.deliver(made);
    });
}

}  // namespace

mpc_status profile_on_device(mpc_context* c, const uint16_t* d_counts, const mpc_basis_choice* d_choices, const double* quant,
                             const uint8_t* d_rgb, int width, int height, uint32_t* d_profile, int* d_error, hipStream_t s) {
    CallQuant cq;
    if (const mpc_status qs = header_quant_device(c, quant, s, &cq); qs != MPC_OK) return qs;
    mpc::ProfileParams p{};
    p.counts = d_counts;
    p.choices = reinterpret_cast<const uint32_t*>(d_choices);
    p.quant = cq.d_q;
    p.K = c->K;
    p.width = width;
    p.height = height;
    p.tiles_x = (width + 7) / 8;
    p.tiles_y = (height + 7) / 8;
    p.original = d_rgb;
    p.profile = d_profile;
    p.error = d_error;
    p.fast = c->fast ? 1 : 0;
    const int err = mpc::launch_depth_profile(dict_device(c), p, s);
    if (err != 0) return launch_failed(err);
    return MPC_OK;
}

mpc_status multiplier_search(const std::function<mpc_status(int, bool*)>& probe, const std::function<mpc_status()>& behind_first, int* found) {
    *found = -1;
    bool fits = false;
    if (const mpc_status ps = probe(mpc::kBudgetLambdas - 1, &fits); ps != MPC_OK) return ps;
    if (const mpc_status bs = behind_first(); bs != MPC_OK) return bs;
    if (!fits) return MPC_OK;
    // lo infeasible (-1: the full result), hi feasible
    int lo = -1, hi = mpc::kBudgetLambdas - 1;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;                             // lo + hi >= -1 + 1: the shift rounds down
        if (const mpc_status ps = probe(mid, &fits); ps != MPC_OK) return ps;
        if (fits) hi = mid;
        else lo = mid;
    }
    *found = hi;
    return MPC_OK;
}

extern "C" {

int mpc_budget_lambda(int j, uint64_t* lambda) {
    if (!lambda || j < 0 || j >= mpc::kBudgetLambdas) return fail(MPC_ERR_ARGUMENT, "multiplier %d: 0 to %d", j, mpc::kBudgetLambdas - 1);
    *lambda = mpc::budget_lambda(j);
    return MPC_OK;
}

mpc_status mpc_budget_weights(const uint8_t* index, size_t index_bytes, uint32_t* weights) {
    return guarded([&]() -> mpc_status {
        if (!index || !weights) return fail(MPC_ERR_ARGUMENT, "null argument");
        const int verdict = mpc::budget_weights(index, index_bytes, weights);
        if (verdict == 1) return fail(MPC_ERR_BITSTREAM, "not a seek index");
        if (verdict == 2) return fail(MPC_ERR_ARGUMENT, "a serial-only index holds no stream sizes");
        return MPC_OK;
    });
}

mpc_status mpc_budget_allocate(const uint32_t* profile, const uint16_t* counts, long long tiles, int K, const uint32_t* weights, int j,
                               uint8_t* depth, uint16_t* out_counts, uint64_t* totals) {
    return guarded([&]() -> mpc_status {
        if (!profile || !counts || !weights || !totals) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (tiles < 0 || K < 1 || K > MPC_MAX_K || j < 0 || j >= mpc::kBudgetLambdas) return fail(MPC_ERR_ARGUMENT, "tiles %lld, K %d, multiplier %d", tiles, K, j);
        mpc::budget_allocate(profile, counts, tiles, K, weights, j, depth, out_counts, totals);
        return MPC_OK;
    });
}

mpc_status mpc_depth_profile_device(mpc_context* c, const uint16_t* d_counts, const mpc_basis_choice* d_choices, const double* quant,
                                    const uint8_t* d_rgb, int width, int height, uint32_t* d_profile, void* stream) {
    return guarded([&]() -> mpc_status {
        if (!c || !d_counts || !d_choices || !d_rgb || !d_profile) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (c->device < 0) return no_device();
        long long tiles = 0;
        if (const mpc_status gs = geometry(width, height, &tiles); gs != MPC_OK) return gs;
        HIP_TRY(hipSetDevice(c->device));
        if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
        if (const mpc_status fs = crop_flag(c); fs != MPC_OK) return fs;
        return profile_on_device(c, d_counts, d_choices, quant, d_rgb, width, height, d_profile, c->d_crop_flag, static_cast<hipStream_t>(stream));
    });
}

mpc_status mpc_budget_allocate_emphasis_device(mpc_context* c, const uint32_t* d_profile, const uint16_t* d_counts, const uint8_t* d_emphasis,
                                               long long tiles, const uint32_t* weights, int j, uint8_t* d_depth, uint16_t* d_out_counts,
                                               unsigned long long* d_totals, void* stream) {
    return guarded([&]() -> mpc_status {
        if (!c || !d_profile || !d_counts || !weights || !d_depth || !d_out_counts || !d_totals) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (c->device < 0) return no_device();
        if (tiles < 1 || tiles * 3 >= (1LL << 31) || j < 0 || j >= mpc::kBudgetLambdas) return fail(MPC_ERR_ARGUMENT, "tiles %lld, multiplier %d", tiles, j);
        HIP_TRY(hipSetDevice(c->device));
        if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
        return allocate_on_device(c, d_profile, d_counts, d_emphasis, tiles, weights, j, d_depth, d_out_counts, d_totals, static_cast<hipStream_t>(stream));
    });
}

mpc_status mpc_budget_allocate_device(mpc_context* c, const uint32_t* d_profile, const uint16_t* d_counts, long long tiles, const uint32_t* weights,
                                      int j, uint8_t* d_depth, uint16_t* d_out_counts, unsigned long long* d_totals, void* stream) {
    return mpc_budget_allocate_emphasis_device(c, d_profile, d_counts, nullptr, tiles, weights, j, d_depth, d_out_counts, d_totals, stream);
}

mpc_status mpc_encode_image_budget(mpc_context* c, const uint8_t* rgb, int width, int height, const double* quant, size_t budget, int index_interval,
                                   uint8_t** bytes, size_t* nbytes, uint8_t** index, size_t* index_bytes, uint8_t* depth, mpc_budget_info* info) {
    return encode_budget(c, rgb, false, nullptr, width, height, quant, budget, index_interval, bytes, nbytes, index, index_bytes, depth, info);
}

mpc_status mpc_encode_image_budget_device(mpc_context* c, const uint8_t* d_rgb, int width, int height, const double* quant, size_t budget,
                                          int index_interval, uint8_t** bytes, size_t* nbytes, uint8_t** index, size_t* index_bytes, uint8_t* depth,
                                          mpc_budget_info* info) {
    return encode_budget(c, d_rgb, true, nullptr, width, height, quant, budget, index_interval, bytes, nbytes, index, index_bytes, depth, info);
}

mpc_status mpc_budget_sweep(const uint32_t* profile, const uint16_t* counts, long long tiles, int K, const uint32_t* weights, uint64_t* totals) {
    return guarded([&]() -> mpc_status {
        if (!profile || !counts || !weights || !totals) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (tiles < 0 || K < 1 || K > MPC_MAX_K) return fail(MPC_ERR_ARGUMENT, "tiles %lld, K %d", tiles, K);
        mpc::budget_sweep(profile, counts, tiles, K, weights, totals);
        return MPC_OK;
    });
}

int mpc_quality_pick(const uint64_t* totals, uint64_t max_sse) { return totals ? mpc::quality_pick(totals, max_sse) : -1; }

mpc_status mpc_sse_for_psnr(double psnr, int width, int height, uint64_t* max_sse) {
    return guarded([&]() -> mpc_status {
        if (!max_sse) return fail(MPC_ERR_ARGUMENT, "null argument");
        long long tiles = 0;
        if (const mpc_status gs = geometry(width, height, &tiles); gs != MPC_OK) return gs;
        if (std::isnan(psnr) || (std::isinf(psnr) && psnr < 0)) return fail(MPC_ERR_ARGUMENT, "a PSNR of %g", psnr);
        const uint64_t limit = uint64_t{195075} * 64 * static_cast<uint64_t>(tiles);                                     // 3 * 255^2 a pixel
        *max_sse = mpc::sse_for_psnr(psnr, limit, [&](uint64_t s) { return mpc::psnr_from_sse(static_cast<double>(s), width, height); });
        return MPC_OK;
    });
}

mpc_status mpc_budget_sweep_emphasis_device(mpc_context* c, const uint32_t* d_profile, const uint16_t* d_counts, const uint8_t* d_emphasis,
                                            long long tiles, const uint32_t* weights, unsigned long long* d_totals, void* stream) {
    return guarded([&]() -> mpc_status {
        if (!c || !d_profile || !d_counts || !weights || !d_totals) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (c->device < 0) return no_device();
        if (tiles < 1 || tiles * 3 >= (1LL << 31)) return fail(MPC_ERR_ARGUMENT, "tiles %lld", tiles);
        HIP_TRY(hipSetDevice(c->device));
        if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
        return sweep_on_device(c, d_profile, d_counts, d_emphasis, tiles, weights, d_totals, static_cast<hipStream_t>(stream));
    });
}

mpc_status mpc_budget_sweep_device(mpc_context* c, const uint32_t* d_profile, const uint16_t* d_counts, long long tiles, const uint32_t* weights,
                                   unsigned long long* d_totals, void* stream) {
    return mpc_budget_sweep_emphasis_device(c, d_profile, d_counts, nullptr, tiles, weights, d_totals, stream);
}

mpc_status mpc_encode_image_quality(mpc_context* c, const uint8_t* rgb, int width, int height, const double* quant, unsigned long long max_sse,
                                    int index_interval, uint8_t** bytes, size_t* nbytes, uint8_t** index, size_t* index_bytes, uint8_t* depth,
                                    mpc_quality_info* info) {
    return encode_quality(c, rgb, false, nullptr, width, height, quant, max_sse, index_interval, bytes, nbytes, index, index_bytes, depth, info);
}

mpc_status mpc_encode_image_quality_device(mpc_context* c, const uint8_t* d_rgb, int width, int height, const double* quant,
                                           unsigned long long max_sse, int index_interval, uint8_t** bytes, size_t* nbytes, uint8_t** index,
                                           size_t* index_bytes, uint8_t* depth, mpc_quality_info* info) {
    return encode_quality(c, d_rgb, true, nullptr, width, height, quant, max_sse, index_interval, bytes, nbytes, index, index_bytes, depth, info);
}

// ---- emphasis maps ----
mpc_status mpc_budget_allocate_emphasis(const uint32_t* profile, const uint16_t* counts, const uint8_t* emphasis, long long tiles, int K,
                                        const uint32_t* weights, int j, uint8_t* depth, uint16_t* out_counts, uint64_t* totals) {
    return guarded([&]() -> mpc_status {
        if (!profile || !counts || !weights || !totals) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (tiles < 0 || K < 1 || K > MPC_MAX_K || j < 0 || j >= mpc::kBudgetLambdas) return fail(MPC_ERR_ARGUMENT, "tiles %lld, K %d, multiplier %d", tiles, K, j);
        mpc::budget_allocate_emphasis(profile, counts, emphasis, tiles, K, weights, j, depth, out_counts, totals);
        return MPC_OK;
    });
}

mpc_status mpc_budget_sweep_emphasis(const uint32_t* profile, const uint16_t* counts, const uint8_t* emphasis, long long tiles, int K,
                                     const uint32_t* weights, uint64_t* totals) {
    return guarded([&]() -> mpc_status {
        if (!profile || !counts || !weights || !totals) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (tiles < 0 || K < 1 || K > MPC_MAX_K) return fail(MPC_ERR_ARGUMENT, "tiles %lld, K %d", tiles, K);
        mpc::budget_sweep_emphasis(profile, counts, emphasis, tiles, K, weights, totals);
        return MPC_OK;
    });
}

namespace {
mpc_status mask_arguments(const void* mask, int width, int height, size_t row_stride, int lo, int hi, const void* emphasis) {
    if (!mask || !emphasis) return fail(MPC_ERR_ARGUMENT, "null argument");
    long long tiles = 0;
    if (const mpc_status gs = geometry(width, height, &tiles); gs != MPC_OK) return gs;
    if (row_stride < static_cast<size_t>(width)) return fail(MPC_ERR_ARGUMENT, "row_stride %zu for %d mask bytes", row_stride, width);
    if (lo < 1 || hi < lo || hi > MPC_EMPHASIS_MAX) return fail(MPC_ERR_ARGUMENT, "emphasis from %d to %d: 1 <= lo <= hi <= %d", lo, hi, MPC_EMPHASIS_MAX);
    return MPC_OK;
}
}  // namespace

mpc_status mpc_emphasis_from_mask(const uint8_t* mask, int width, int height, size_t row_stride, int lo, int hi, uint8_t* emphasis) {
    return guarded([&]() -> mpc_status {
        if (const mpc_status as = mask_arguments(mask, width, height, row_stride, lo, hi, emphasis); as != MPC_OK) return as;
        mpc::emphasis_from_mask(mask, width, height, row_stride, lo, hi, emphasis);
        return MPC_OK;
    });
}

mpc_status mpc_emphasis_from_mask_device(mpc_context* c, const uint8_t* d_mask, int width, int height, size_t row_stride, int lo, int hi,
                                         uint8_t* d_emphasis, void* stream) {
    return guarded([&]() -> mpc_status {
        if (!c) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (const mpc_status as = mask_arguments(d_mask, width, height, row_stride, lo, hi, d_emphasis); as != MPC_OK) return as;
        if (c->device < 0) return no_device();
        HIP_TRY(hipSetDevice(c->device));
        if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
        const int err = mpc::launch_emphasis_mask(d_mask, width, height, row_stride, lo, hi, d_emphasis, stream);
        if (err != 0) return launch_failed(err);
        return MPC_OK;
    });
}

mpc_status mpc_encode_image_budget_emphasis(mpc_context* c, const uint8_t* rgb, const uint8_t* emphasis, int width, int height, const double* quant,
                                            size_t budget, int index_interval, uint8_t** bytes, size_t* nbytes, uint8_t** index, size_t* index_bytes,
                                            uint8_t* depth, mpc_budget_info* info) {
    return encode_budget(c, rgb, false, emphasis, width, height, quant, budget, index_interval, bytes, nbytes, index, index_bytes, depth, info);
}

mpc_status mpc_encode_image_budget_emphasis_device(mpc_context* c, const uint8_t* d_rgb, const uint8_t* d_emphasis, int width, int height,
                                                   const double* quant, size_t budget, int index_interval, uint8_t** bytes, size_t* nbytes,
                                                   uint8_t** index, size_t* index_bytes, uint8_t* depth, mpc_budget_info* info) {
    return encode_budget(c, d_rgb, true, d_emphasis, width, height, quant, budget, index_interval, bytes, nbytes, index, index_bytes, depth, info);
}

mpc_status mpc_encode_image_quality_emphasis(mpc_context* c, const uint8_t* rgb, const uint8_t* emphasis, int width, int height, const double* quant,
                                             unsigned long long max_sse, int index_interval, uint8_t** bytes, size_t* nbytes, uint8_t** index,
                                             size_t* index_bytes, uint8_t* depth, mpc_quality_info* info) {
    return encode_quality(c, rgb, false, emphasis, width, height, quant, max_sse, index_interval, bytes, nbytes, index, index_bytes, depth, info);
}

mpc_status mpc_encode_image_quality_emphasis_device(mpc_context* c, const uint8_t* d_rgb, const uint8_t* d_emphasis, int width, int height,
                                                    const double* quant, unsigned long long max_sse, int index_interval, uint8_t** bytes,
                                                    size_t* nbytes, uint8_t** index, size_t* index_bytes, uint8_t* depth, mpc_quality_info* info) {
    return encode_quality(c, d_rgb, true, d_emphasis, width, height, quant, max_sse, index_interval, bytes, nbytes, index, index_bytes, depth, info);
}

// ---- a group of frames ----
mpc_status mpc_budget_allocate_group(const uint32_t* profile, const uint16_t* counts, const uint8_t* emphasis, int frames, long long tiles, int K,
                                     const uint32_t* weights, int j, uint8_t* depth, uint16_t* out_counts, uint64_t* totals) {
    return guarded([&]() -> mpc_status {
        if (!profile || !counts || !weights || !totals) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (frames < 1 || frames > MPC_GROUP_MAX_FRAMES) return fail(MPC_ERR_ARGUMENT, "%d frames: 1 to %d", frames, MPC_GROUP_MAX_FRAMES);
        if (tiles < 0 || K < 1 || K > MPC_MAX_K || j < 0 || j >= mpc::kBudgetLambdas) return fail(MPC_ERR_ARGUMENT, "tiles %lld, K %d, multiplier %d", tiles, K, j);
        mpc::budget_allocate_group(profile, counts, emphasis, frames, tiles, K, weights, j, depth, out_counts, totals);
        return MPC_OK;
    });
}

mpc_status mpc_budget_sweep_group(const uint32_t* profile, const uint16_t* counts, const uint8_t* emphasis, int frames, long long tiles, int K,
                                  const uint32_t* weights, uint64_t* totals) {
    return guarded([&]() -> mpc_status {
        if (!profile || !counts || !weights || !totals) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (frames < 1 || frames > MPC_GROUP_MAX_FRAMES) return fail(MPC_ERR_ARGUMENT, "%d frames: 1 to %d", frames, MPC_GROUP_MAX_FRAMES);
        if (tiles < 0 || K < 1 || K > MPC_MAX_K) return fail(MPC_ERR_ARGUMENT, "tiles %lld, K %d", tiles, K);
        mpc::budget_sweep_group(profile, counts, emphasis, frames, tiles, K, weights, totals);
        return MPC_OK;
    });
}

mpc_status mpc_sse_for_psnr_group(double psnr, int width, int height, int frames, uint64_t* max_sse) {
    return guarded([&]() -> mpc_status {
        if (!max_sse) return fail(MPC_ERR_ARGUMENT, "null argument");
        long long tiles = 0;
        if (const mpc_status gs = geometry(width, height, &tiles); gs != MPC_OK) return gs;
        if (frames < 1 || frames > MPC_GROUP_MAX_FRAMES) return fail(MPC_ERR_ARGUMENT, "%d frames: 1 to %d", frames, MPC_GROUP_MAX_FRAMES);
        if (std::isnan(psnr) || (std::isinf(psnr) && psnr < 0)) return fail(MPC_ERR_ARGUMENT, "a PSNR of %g", psnr);
        const uint64_t limit = uint64_t{195075} * 64 * static_cast<uint64_t>(tiles) * static_cast<uint64_t>(frames);     // 3 * 255^2 a pixel
        const size_t pixels = static_cast<size_t>(width) * static_cast<size_t>(height) * static_cast<size_t>(frames);
        *max_sse = mpc::sse_for_psnr(psnr, limit, [&](uint64_t s) { return mpc::psnr_from_sse_pixels(static_cast<double>(s), pixels); });
        return MPC_OK;
    });
}

mpc_status mpc_budget_allocate_group_device(mpc_context* c, const uint32_t* d_profile, const uint16_t* d_counts, const uint8_t* d_emphasis, int frames,
                                            long long tiles, const uint32_t* weights, int j, uint8_t* d_depth, uint16_t* d_out_counts,
                                            unsigned long long* d_totals, void* stream) {
    return guarded([&]() -> mpc_status {
        if (!c || !d_profile || !d_counts || !weights || !d_depth || !d_out_counts || !d_totals) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (c->device < 0) return no_device();
        if (const mpc_status gs = group_arguments(frames, tiles); gs != MPC_OK) return gs;
        if (j < 0 || j >= mpc::kBudgetLambdas) return fail(MPC_ERR_ARGUMENT, "multiplier %d", j);
        HIP_TRY(hipSetDevice(c->device));
        if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
        return allocate_group_on_device(c, d_profile, d_counts, d_emphasis, frames, tiles, weights, j, d_depth, d_out_counts, d_totals,
                                        static_cast<hipStream_t>(stream));
    });
}

mpc_status mpc_budget_sweep_group_device(mpc_context* c, const uint32_t* d_profile, const uint16_t* d_counts, const uint8_t* d_emphasis, int frames,
                                         long long tiles, const uint32_t* weights, unsigned long long* d_totals, void* stream) {
    return guarded([&]() -> mpc_status {
        if (!c || !d_profile || !d_counts || !weights || !d_totals) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (c->device < 0) return no_device();
        if (const mpc_status gs = group_arguments(frames, tiles); gs != MPC_OK) return gs;
        HIP_TRY(hipSetDevice(c->device));
        if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
        return sweep_group_on_device(c, d_profile, d_counts, d_emphasis, frames, tiles, weights, d_totals, static_cast<hipStream_t>(stream));
    });
}

mpc_status mpc_encode_images_budget(mpc_context* c, const uint8_t* const* frames, const uint8_t* emphasis, int n_frames, int width, int height,
                                    const double* quant, size_t budget, int index_interval, uint8_t** bytes, size_t* nbytes, uint8_t** indexes,
                                    size_t* index_bytes, uint8_t* depth, mpc_budget_info* frame_info, mpc_budget_info* info) {
    return encode_group_budget(c, frames, false, emphasis, n_frames, width, height, quant, budget, index_interval, bytes, nbytes, indexes, index_bytes,
                               depth, frame_info, info);
}

mpc_status mpc_encode_images_budget_device(mpc_context* c, const uint8_t* const* d_frames, const uint8_t* d_emphasis, int n_frames, int width,
                                           int height, const double* quant, size_t budget, int index_interval, uint8_t** bytes, size_t* nbytes,
                                           uint8_t** indexes, size_t* index_bytes, uint8_t* depth, mpc_budget_info* frame_info,
                                           mpc_budget_info* info) {
    return encode_group_budget(c, d_frames, true, d_emphasis, n_frames, width, height, quant, budget, index_interval, bytes, nbytes, indexes,
                               index_bytes, depth, frame_info, info);
}

mpc_status mpc_encode_images_quality(mpc_context* c, const uint8_t* const* frames, const uint8_t* emphasis, int n_frames, int width, int height,
                                     const double* quant, unsigned long long max_sse, int index_interval, uint8_t** bytes, size_t* nbytes,
                                     uint8_t** indexes, size_t* index_bytes, uint8_t* depth, mpc_quality_info* frame_info, mpc_quality_info* info) {
    return encode_group_quality(c, frames, false, emphasis, n_frames, width, height, quant, max_sse, index_interval, bytes, nbytes, indexes,
                                index_bytes, depth, frame_info, info);
}

mpc_status mpc_encode_images_quality_device(mpc_context* c, const uint8_t* const* d_frames, const uint8_t* d_emphasis, int n_frames, int width,
                                            int height, const double* quant, unsigned long long max_sse, int index_interval, uint8_t** bytes,
                                            size_t* nbytes, uint8_t** indexes, size_t* index_bytes, uint8_t* depth, mpc_quality_info* frame_info,
                                            mpc_quality_info* info) {
    return encode_group_quality(c, d_frames, true, d_emphasis, n_frames, width, height, quant, max_sse, index_interval, bytes, nbytes, indexes,
                                index_bytes, depth, frame_info, info);
}

}  // extern "C"
