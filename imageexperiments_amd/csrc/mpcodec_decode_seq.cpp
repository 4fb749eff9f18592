// mpcodec_decode_seq.cpp -- product: the C ABI's decoder of containers: mpc_decode_image, mpc_decode_images, mpc_decode_images_device,
// mpc_decode_image_device, all one call of decode_sequence.  Nothing in the format is serial BETWEEN frames, so the containers of a
// call are parsed side by side on threads of the call's own (a call of one frame: on the calling thread), each doing only what the
// format chains from code to code (mpc::read_compressed_coded: the entropy codes).  The coded streams cross PCIe and the per-symbol
// rest -- run-length expansion, DC sums -- happens on the device (mp_unpack.hip) in front of the gather and the reconstruction,
// frames pipelined over slots of their own streams.  A frame that comes with a seek index (mpc_decode_images_indexed*) skips the
// serial parse: its container's bytes go up as they are and the device undoes the entropy codes chunk by chunk (mp_parse.hip)
// into the same buffers; whatever makes the index unusable sends the frame down the serial route from the start.  A call that wants
// a pixel rectangle of each frame (mpc_decode_regions_indexed*) is one more caller of the same sequence: with an index the window's
// share of every stage behind the lengths stream (route 0), without one the whole frame by the serial route and a 2-D copy (route 1).
// A view (mpc_decode_views_indexed*) is a region with a cap on the pursuit steps and a reduction: the streams of the steps it does
// not want are empty in the host's tables, the lengths are cut behind their check, and mp_decode_view_kernel ends either route.
#include <algorithm>
#include <atomic>
#include <climits>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>

#include "mpc_internal.h"

namespace {

// What the unpack kernels need to know of the 6K streams, from sizes the host has in hand; false = sizes beyond what they index
struct UnpackPlan {
    std::vector<mpc::UnpackStream> table;       // [6K + 1]
    size_t n_coded = 0, n_symbols = 0;
    unsigned n_blocks = 0;
    int dc_stream[3] = {};
    unsigned dc_blk_begin[4] = {};
};

template <class Len>
bool plan_unpack(int K, Len coded_len, const uint8_t* is_packed, const unsigned long long* expect_ull, const size_t* expect_sz,
                 UnpackPlan& p) {
    const int n = 6 * K;
    p.table.assign(static_cast<size_t>(n) + 1, mpc::UnpackStream{});
    unsigned long long coded_at = 0, out_at = 0, blocks = 0;
    constexpr unsigned long long kLimit = 1ULL << 40;               // symbols; far beyond any frame, far from overflow
    for (int i = 0; i < n; ++i) {
        const unsigned long long len = coded_len(i), expect = expect_ull ? expect_ull[i] : expect_sz[i];
        if (len > kLimit || expect > kLimit) return false;
        mpc::UnpackStream& s = p.table[i];
        s.coded_off = coded_at;
        s.coded_len = len;
        s.expect = expect;
        s.out_off = out_at;
        s.blk_begin = static_cast<unsigned>(blocks);
        s.flags = is_packed[i] ? mpc::kUnpackPacked : 0u;
        coded_at += len;
        out_at += expect;
        blocks += (len + mpc::kUnpackBlock - 1) / mpc::kUnpackBlock;
        if (coded_at > kLimit || out_at > kLimit || blocks > 0x7FFFFFFFull) return false;
    }
    p.table[n].coded_off = coded_at;
    p.table[n].out_off = out_at;
    p.table[n].blk_begin = static_cast<unsigned>(blocks);
    p.n_coded = static_cast<size_t>(coded_at);
    p.n_symbols = static_cast<size_t>(out_at);
    p.n_blocks = static_cast<unsigned>(blocks);
    unsigned long long dc_blocks = 0;
    for (int ch = 0; ch < 3; ++ch) {
        p.dc_stream[ch] = 2 * K * ch + 1;
        p.dc_blk_begin[ch] = static_cast<unsigned>(dc_blocks);
        dc_blocks += (p.table[p.dc_stream[ch]].expect + mpc::kUnpackBlock - 1) / mpc::kUnpackBlock;
    }
    p.dc_blk_begin[3] = static_cast<unsigned>(dc_blocks);
    return true;
}

// the unpack kernels' output and scratch in a device buffer; a->coded and a->streams are the caller's
void carve_unpack(Carve& cv, const UnpackPlan& p, int K, mpc::UnpackArgs* a) {
    a->n_streams = 6 * K;
    a->n_blocks = p.n_blocks;
    a->error = cv.take<int>(3);                                     // [1]: the reconstruction's error word, [2]: the device parse's
    a->symbols = cv.take<uint16_t>(p.n_symbols + 2);                // the kernels touch whole words: an even number of symbols
    a->blk_piece = cv.take<unsigned>(4 * static_cast<size_t>(p.n_blocks) + 4);
    a->blk_entry = cv.take<unsigned>(static_cast<size_t>(p.n_blocks) + 1);
    a->blk_out = cv.take<unsigned long long>(static_cast<size_t>(p.n_blocks) + 1);
    a->stream_ok = cv.take<unsigned>(6 * static_cast<size_t>(K));
    a->dc_part = cv.take<unsigned>(static_cast<size_t>(p.dc_blk_begin[3]) + 1);
    for (int ch = 0; ch < 3; ++ch) a->dc_stream[ch] = p.dc_stream[ch];
    for (int k = 0; k < 4; ++k) a->dc_blk_begin[k] = p.dc_blk_begin[k];
}

// ---- the sequence ----
struct ComposeTarget;                           // below, with paste_on_slot
struct Sequence {
    mpc_context* c = nullptr;
    Tuning tuning;
    int n = 0, slots = 0;
    bool single = false;                        // mpc_decode_image: the error text carries no "frame 0: "
    const uint8_t* const* bytes = nullptr;
    const size_t* nbytes = nullptr;
    uint8_t** rgb = nullptr;                    // host form: the results
    uint8_t* const* d_rgb = nullptr;            // device form: the caller's buffers
    const size_t* capacity = nullptr;
    const uint8_t* const* indexes = nullptr;    // optional, and optional per frame: the seek index of frame f
    const size_t* index_bytes = nullptr;
    int* routes = nullptr;                      // optional: per frame 0 = parsed on the device, 1 = the serial route
    bool scan = false;                          // mpc_decode_images_scan*: no index comes with a frame; the device scan proposes one
    uint8_t** out_indexes = nullptr;            // ... optional: the version-1 blob of every frame on route 0 (malloc), else NULL
    size_t* out_index_bytes = nullptr;
    const mpc_rect* rects = nullptr;            // mpc_decode_regions_indexed*: the rectangle wanted of frame f
    bool parse_all = false;                     // ... MPC_REGION_PARSE_ALL
    const mpc_view* views = nullptr;            // mpc_decode_views_indexed*: steps and reduction of frame f; rects[f] is then its rectangle, resolved
    int* width = nullptr;
    int* height = nullptr;
    // mpc_transcode_views_indexed: no pixels; behind the gather the crop kernel and the records-to-container chain on the job slot
    // of the decode slot's number leave frame f's container here (malloc)
    uint8_t** containers = nullptr;
    size_t* container_bytes = nullptr;
    const ComposeTarget* compose = nullptr;      // mpc_compose_indexed: frame f is a container part; no pixels, no container of its own
    std::atomic<int> next{0};                   // frames are handed out in order
    std::mutex lock;
    std::condition_variable turn;
    long long slot_uses[mpc_context::kDecodeSlots] = {};   // frame f owns slot f % slots once it has been used f / slots times
    int failed_frame = INT_MAX;                 // the first failing frame, its status and text
    mpc_status failed_status = MPC_OK;
    std::string failed_text;

    // the bytes frame f's pixels take at the caller's, the frame being width x height
    size_t out_bytes(int f, int width, int height) const {
        if (containers || compose) return 0;
        if (views)
            return static_cast<size_t>(view_extent(rects[f].width, views[f].scale_log2)) *
                   static_cast<size_t>(view_extent(rects[f].height, views[f].scale_log2)) * 3;
        if (rects) return static_cast<size_t>(rects[f].width) * static_cast<size_t>(rects[f].height) * 3;
        return static_cast<size_t>(width) * height * 3;
    }
    bool failed_before(int f) {
        std::lock_guard<std::mutex> hold(lock);
        return failed_frame < f;
    }
    void record_failure(int f, mpc_status st) {
        next.store(n);                          // hand out no more frames; those taken finish or skip
        std::lock_guard<std::mutex> hold(lock);
        if (f < failed_frame) {
            failed_frame = f;
            failed_status = st;
            failed_text = mpc_last_error();
        }
    }
};

// One upload-and-unpack on a decode slot: the coded streams and the caller's own pieces through the slot's pinned buffer to the
// device, the unpack kernels behind them on the slot's stream.  The caller sets the first block of fields.
struct UnpackJob {
    const UnpackPlan* plan = nullptr;
    int K = 0;
    const uint16_t* streams[6 * MPC_MAX_K] = {};    // the coded streams on the host, plan->table[i].coded_len symbols each
    const void* extra[2] = {};                      // uploaded with them (the frame decoder's counts and quantiser steps)
    size_t extra_bytes[2] = {};
    size_t behind_bytes = 0;                        // device bytes the caller carves behind the unpack kernels' buffers
    size_t result_bytes = 0;                        // what the caller brings back through `h_result`
    bool pooled = false, trace = false;             // copy on the worker pool; stamp the slot's events 0 - 2
    // set by upload_and_unpack
    int* h_flags = nullptr;                         // pinned, preset to -1: where the caller copies ua.error[0..1] back to
    char* h_result = nullptr;                       // pinned: free once the upload has left it (stream order)
    const void* d_extra[2] = {};
    char* d_behind = nullptr;
    const unsigned long long* d_aux = nullptr;      // upload_and_parse(with_aux): the index's aux entries and every stream's first
    const unsigned long long* d_aux_off = nullptr;
    mpc::UnpackArgs ua{};
    double staged_ms = 0.0;                         // trace_ms() with everything in pinned memory, nothing enqueued yet
};

mpc_status upload_and_unpack(DecodeSlot& slot, UnpackJob& j) {
    const UnpackPlan& plan = *j.plan;
    const int n = 6 * j.K;
    constexpr size_t kHead = 256;                                   // the pinned buffer's head: the two error words coming back
    uint16_t* coded;
    mpc::UnpackStream* table;
    char* extra[2];
    auto upload_layout = [&](char* base) {                          // the same in pinned memory and on the device
        Carve cv{base};
        coded = cv.take<uint16_t>(plan.n_coded + 2);
        table = cv.take<mpc::UnpackStream>(plan.table.size());
        for (int k = 0; k < 2; ++k) extra[k] = cv.take<char>(j.extra_bytes[k]);
        return cv.at;
    };
    const size_t upload_bytes = upload_layout(nullptr);
    Carve scratch{nullptr, upload_bytes};
    carve_unpack(scratch, plan, j.K, &j.ua);
    const size_t behind_at = scratch.at;
    if (const mpc_status gs = slot.pinned.reserve(kHead + std::max(upload_bytes, Carve::up(j.result_bytes)), "pinned decode staging"); gs != MPC_OK)
        return gs;
    if (const mpc_status gs = slot.dev.reserve(behind_at + j.behind_bytes, "device decode staging"); gs != MPC_OK) return gs;
    j.h_flags = reinterpret_cast<int*>(slot.pinned.data());
    j.h_result = slot.pinned.data() + kHead;
    upload_layout(j.h_result);
    const auto stage = [&](int job) {
        if (job < 2) {
            if (j.extra_bytes[job]) std::memcpy(extra[job], j.extra[job], j.extra_bytes[job]);
        } else if (const mpc::UnpackStream& s = plan.table[job - 2]; s.coded_len)
            std::memcpy(coded + s.coded_off, j.streams[job - 2], sizeof(uint16_t) * s.coded_len);
    };
    if (j.pooled) mpc::parallel_jobs(n + 2, stage);
    else
        for (int job = 0; job < n + 2; ++job) stage(job);
    std::memcpy(table, plan.table.data(), sizeof(mpc::UnpackStream) * plan.table.size());
    j.h_flags[0] = j.h_flags[1] = -1;
    char* dbase = slot.dev.data();
    upload_layout(dbase);                                           // coded, table, extra: their device copies now
    scratch = Carve{dbase, upload_bytes};
    carve_unpack(scratch, plan, j.K, &j.ua);
    j.ua.coded = coded;
    j.ua.streams = table;
    for (int k = 0; k < 2; ++k) j.d_extra[k] = extra[k];
    j.d_behind = dbase + behind_at;
    j.staged_ms = trace_ms();
    hipStream_t st = slot.stream;
    if (j.trace) HIP_TRY(hipEventRecord(slot.stamp[0], st));
    HIP_TRY(hipMemsetAsync(j.ua.error, 0, 3 * sizeof(int), st));
    HIP_TRY(hipMemcpyAsync(dbase, j.h_result, upload_bytes, hipMemcpyHostToDevice, st));
    if (j.trace) HIP_TRY(hipEventRecord(slot.stamp[1], st));
    if (const int e = mpc::launch_unpack(j.ua, st); e != 0) return launch_failed(e);
    if (j.trace) HIP_TRY(hipEventRecord(slot.stamp[2], st));
    return MPC_OK;
}

// ---- the indexed route: the container's bytes up, the entropy codes undone on the device ----
// What the parse kernels need, from an index the host has checked against its container (mpc::plan_indexed_parse)
struct ParsePlan {
    mpc::IndexedPlan ip;
    std::vector<mpc::ParseStream> streams;      // [6K + 2]
    std::vector<uint32_t> luts, lens;
    std::vector<uint16_t> tables;
    size_t n_checkpoints = 0, n_counts = 0;
    unsigned n_groups = 0;
    UnpackPlan unpack;
    // index version 2: the aux entries as in the blob, two words each, stream behind stream, and per stream of the 6K its first
    // entry (~0: none).  Used by a region decode alone
    bool expanded = false;
    std::vector<unsigned long long> aux, aux_off;
};

// A Huffman stream's tables as the parse and scan kernels read them, appended to the uploads: the window table (symbol | length << 16
// | pseudo-EOF), and for codes longer than the window the per-length rows and the entry -> symbol table
void append_code_tables(const mpc::HuffmanCodebook& cb, mpc::ParseStream& ps, std::vector<uint32_t>& luts, std::vector<uint32_t>& lens,
                        std::vector<uint16_t>& tables) {
    constexpr size_t kLut = size_t(1) << mpc::kParseLutBits;
    const uint32_t eof = static_cast<uint32_t>(cb.total) - 1u;
    ps.total = cb.total;
    ps.max_length = static_cast<unsigned>(cb.max_length);
    ps.lut_off = static_cast<unsigned>(luts.size());
    luts.resize(luts.size() + kLut);
    uint32_t* lut = luts.data() + ps.lut_off;
    for (size_t k = 0; k < kLut; ++k) {                         // (entry << 5) | length -> symbol | length << 16 | pseudo-EOF
        const uint32_t hit = cb.lut[k];
        if (hit) lut[k] = cb.table[hit >> 5] | ((hit & 31u) << 16) | ((hit >> 5) == eof ? mpc::kParseLutEof : 0u);
    }
    if (cb.max_length <= mpc::kParseLutBits) return;            // the window resolves every code: no per-length test, no entry table
    ps.len_off = static_cast<unsigned>(lens.size());
    lens.resize(lens.size() + 3 * 33, 0);
    for (int l = 1; l <= cb.max_length; ++l) {
        uint32_t* row = lens.data() + ps.len_off + 3 * l;
        row[0] = cb.counts[l - 1];
        row[1] = cb.first_code[l];
        row[2] = cb.first_index[l];
    }
    ps.table_off = static_cast<unsigned>(tables.size());
    tables.insert(tables.end(), cb.table.begin(), cb.table.end());
}

// false = the index is not used (the serial route decides what becomes of the frame)
// keep_steps (a view; 0 or >= K: every step): a stream of a step at or above it is EMPTY in every table the kernels bound themselves
// by -- no coded symbols, no chunks, no groups, no expanded symbols, no aux entries -- so it is neither parsed, unpacked nor
// gathered, and the streams behind it move up.  ParseStream::expect alone stays the index's: mp_parse_verify_kernel compares it
// with the sizes the uncut lengths give
bool plan_parse(const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes, bool pooled, ParsePlan& p, int keep_steps = 0) {
    if (!mpc::plan_indexed_parse(bytes, nbytes, index, index_bytes, p.ip, pooled)) return false;
    const mpc::ContainerIndex& x = p.ip.index;
    const int K = x.K, n = 6 * K;
    if (K < 1 || K > MPC_MAX_K) return false;
    const auto is_cut = [&](int i) { return keep_steps > 0 && (i % (2 * K)) / 2 >= keep_steps; };      // stream i of the 6K
    std::vector<uint8_t> is_packed(static_cast<size_t>(n));
    std::vector<unsigned long long> expect(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) {
        is_packed[i] = is_cut(i) ? uint8_t(0) : static_cast<uint8_t>(x.streams[static_cast<size_t>(i) + 1].packed);
        expect[i] = is_cut(i) ? 0ull : x.streams[static_cast<size_t>(i) + 1].expect;
    }
    if (!plan_unpack(K, [&](int i) { return is_cut(i) ? 0ull : static_cast<unsigned long long>(x.streams[static_cast<size_t>(i) + 1].n_coded); },
                     is_packed.data(), expect.data(), nullptr, p.unpack))
        return false;
    p.n_counts = 3 * p.ip.tiles;
    p.streams.assign(x.streams.size() + 1, mpc::ParseStream{});
    unsigned long long groups = 0, checkpoints = 0;
    for (size_t j = 0; j < x.streams.size(); ++j) {
        const mpc::IndexStream& is = x.streams[j];
        const mpc::StreamWrapper& w = p.ip.wrappers[j];
        mpc::ParseStream& ps = p.streams[j];
        if (is.checkpoints.size() > 0xFFFFFFFFull) return false;
        const bool cut_away = j != 0 && is_cut(static_cast<int>(j) - 1);
        const size_t chunks = cut_away ? 0 : is.checkpoints.size();
        ps.out_off = j == 0 ? 0 : p.unpack.table[j - 1].coded_off;
        ps.n_coded = cut_away ? 0 : is.n_coded;
        ps.end_bit = is.end_bit;
        ps.cp_off = checkpoints;
        ps.expect = is.expect;
        ps.n_chunks = static_cast<unsigned>(chunks);
        ps.group_begin = static_cast<unsigned>(groups);
        ps.flags = (w.mode == 1 ? mpc::kParseGolomb : 0u) | (j == 0 ? mpc::kParseLengths : 0u);
        ps.m = w.m;
        checkpoints += is.checkpoints.size();                       // the upload holds every stream's: cp_off is the blob's
        groups += (chunks + mpc::kParseGroup - 1) / mpc::kParseGroup;
        if (groups > 0x7FFFFFFFull) return false;
        if (w.mode != 0 || ps.n_chunks == 0) continue;
        append_code_tables(w.cb, ps, p.luts, p.lens, p.tables);
    }
    p.expanded = x.version == 2;
    if (p.expanded) {
        p.aux_off.assign(static_cast<size_t>(n), ~0ull);
        for (int i = 0; i < n; ++i) {
            const mpc::IndexStream& is = x.streams[static_cast<size_t>(i) + 1];
            if (is.aux.empty() || is_cut(i)) continue;              // read_container_index: else one entry per checkpoint
            p.aux_off[i] = p.aux.size() / 2;
            for (const mpc::IndexAux& a : is.aux) {
                p.aux.push_back(a.out);
                p.aux.push_back(static_cast<unsigned long long>(a.prev) | (static_cast<unsigned long long>(a.dc) << 16) |
                                (static_cast<unsigned long long>(a.state) << 32));
            }
        }
    }
    p.streams.back().group_begin = static_cast<unsigned>(groups);
    p.n_groups = static_cast<unsigned>(groups);
    p.n_checkpoints = static_cast<size_t>(checkpoints);
    return true;
}

// upload_and_unpack's counterpart: the container, the checkpoints and the code tables through the slot's pinned buffer to the
// device, the parse kernels behind them; they leave the coded streams and the lengths where upload_and_unpack puts them
// (j.ua.coded, j.d_extra[0]).  j.extra[0] is not used; the unpack kernels are the caller's to launch.  stamp[5]: behind the parse
// deferred: the parse kernels are the caller's to launch as well, from *deferred (a frame of which a window is wanted)
// with_aux: the aux entries of a version-2 index go up behind everything else (j.d_aux, j.d_aux_off); without it the upload is
// what it is for a version-1 index
// words_resident: the scan route has put this container at the head of the slot's device buffer (DeviceStreamScanner::begin, the
// same place and padding); unless the buffer has to grow now, the container is not uploaded a second time
mpc_status upload_and_parse(DecodeSlot& slot, UnpackJob& j, const ParsePlan& pp, const uint8_t* bytes, size_t nbytes,
                            mpc::ParseArgs* deferred = nullptr, bool with_aux = false, bool words_resident = false) {
    const UnpackPlan& plan = *j.plan;
    constexpr size_t kHead = 256;
    const size_t padded = ((nbytes + 3) & ~static_cast<size_t>(3)) + 16;      // a lane's window reads up to 12 bytes behind the last bit
    uint8_t* words;
    unsigned long long* checkpoints;
    mpc::ParseStream* streams;
    uint32_t *luts, *lens;
    uint16_t* tables;
    mpc::UnpackStream* table;
    char* extra;
    unsigned long long *aux = nullptr, *aux_off = nullptr;
    auto upload_layout = [&](char* base) {                          // the same in pinned memory and on the device
        Carve cv{base};
        words = cv.take<uint8_t>(padded);
        checkpoints = cv.take<unsigned long long>(pp.n_checkpoints + 1);
        streams = cv.take<mpc::ParseStream>(pp.streams.size());
        luts = cv.take<uint32_t>(pp.luts.size() + 4);
        lens = cv.take<uint32_t>(pp.lens.size() + 1);
        tables = cv.take<uint16_t>(pp.tables.size() + 1);
        table = cv.take<mpc::UnpackStream>(plan.table.size());
        extra = cv.take<char>(j.extra_bytes[1]);
        if (with_aux) {
            aux = cv.take<unsigned long long>(pp.aux.size() + 2);
            aux_off = cv.take<unsigned long long>(pp.aux_off.size());
        }
        return cv.at;
    };
    const size_t upload_bytes = upload_layout(nullptr);
    mpc::ParseArgs pa{};
    uint16_t* coded;
    auto device_layout = [&](char* base) {                          // behind the upload: the parse kernels' output, then the unpack kernels'
        Carve cv{base, upload_bytes};
        coded = cv.take<uint16_t>(plan.n_coded + 2);
        pa.counts = cv.take<uint16_t>(pp.n_counts + 2);
        pa.hist = cv.take<unsigned>(3 * (mpc::kMaxDeviceK + 1) + 1);
        carve_unpack(cv, plan, j.K, &j.ua);
        return cv.at;
    };
    const size_t behind_at = device_layout(nullptr);
    if (const mpc_status gs = slot.pinned.reserve(kHead + std::max(upload_bytes, Carve::up(j.result_bytes)), "pinned decode staging"); gs != MPC_OK)
        return gs;
    bool dev_grown = false;
    if (const mpc_status gs = slot.dev.reserve(behind_at + j.behind_bytes, "device decode staging", &dev_grown); gs != MPC_OK) return gs;
    const bool keep_words = words_resident && !dev_grown;
    j.h_flags = reinterpret_cast<int*>(slot.pinned.data());
    j.h_result = slot.pinned.data() + kHead;
    upload_layout(j.h_result);
    const size_t piece = size_t(1) << 20, pieces = keep_words ? 0 : (nbytes + piece - 1) / piece;
    const auto stage = [&](int job) {
        const size_t lo = piece * static_cast<size_t>(job), hi = std::min(nbytes, lo + piece);
        std::memcpy(words + lo, bytes + lo, hi - lo);
    };
    if (j.pooled && pieces > 1) mpc::parallel_jobs(static_cast<int>(pieces), stage);
    else
        for (size_t job = 0; job < pieces; ++job) stage(static_cast<int>(job));
    if (!keep_words) std::memset(words + nbytes, 0, padded - nbytes);
    size_t at = 0;
    for (const mpc::IndexStream& is : pp.ip.index.streams) {
        if (!is.checkpoints.empty()) std::memcpy(checkpoints + at, is.checkpoints.data(), sizeof(unsigned long long) * is.checkpoints.size());
        at += is.checkpoints.size();
    }
    std::memcpy(streams, pp.streams.data(), sizeof(mpc::ParseStream) * pp.streams.size());
    if (!pp.luts.empty()) std::memcpy(luts, pp.luts.data(), sizeof(uint32_t) * pp.luts.size());
    if (!pp.lens.empty()) std::memcpy(lens, pp.lens.data(), sizeof(uint32_t) * pp.lens.size());
    if (!pp.tables.empty()) std::memcpy(tables, pp.tables.data(), sizeof(uint16_t) * pp.tables.size());
    std::memcpy(table, plan.table.data(), sizeof(mpc::UnpackStream) * plan.table.size());
    if (j.extra_bytes[1]) std::memcpy(extra, j.extra[1], j.extra_bytes[1]);
    if (with_aux) {
        if (!pp.aux.empty()) std::memcpy(aux, pp.aux.data(), sizeof(unsigned long long) * pp.aux.size());
        std::memcpy(aux_off, pp.aux_off.data(), sizeof(unsigned long long) * pp.aux_off.size());
    }
    j.h_flags[0] = j.h_flags[1] = j.h_flags[2] = -1;
    char* dbase = slot.dev.data();
    upload_layout(dbase);
    device_layout(dbase);
    j.d_aux = aux;
    j.d_aux_off = aux_off;
    pa.words = reinterpret_cast<const uint32_t*>(words);
    pa.checkpoints = checkpoints;
    pa.streams = streams;
    pa.luts = luts;
    pa.lens = lens;
    pa.tables = tables;
    pa.n_streams = static_cast<int>(pp.streams.size()) - 1;
    pa.K = j.K;
    pa.interval = pp.ip.index.interval;
    pa.n_groups = pp.n_groups;
    pa.n_counts = pp.n_counts;
    pa.coded = coded;
    pa.error = j.ua.error + 2;
    j.ua.coded = coded;
    j.ua.streams = table;
    j.d_extra[0] = pa.counts;
    j.d_extra[1] = extra;
    j.d_behind = dbase + behind_at;
    j.staged_ms = trace_ms();
    hipStream_t st = slot.stream;
    if (j.trace) HIP_TRY(hipEventRecord(slot.stamp[0], st));
    HIP_TRY(hipMemsetAsync(j.ua.error, 0, 3 * sizeof(int), st));
    const size_t skip = keep_words ? Carve::up(padded) : 0;          // the container's own piece of the layout
    HIP_TRY(hipMemcpyAsync(dbase + skip, j.h_result + skip, upload_bytes - skip, hipMemcpyHostToDevice, st));
    if (j.trace) HIP_TRY(hipEventRecord(slot.stamp[1], st));
    if (deferred) {
        *deferred = pa;
        return MPC_OK;
    }
    if (const int e = mpc::launch_parse(pa, st); e != 0) return launch_failed(e);
    if (j.trace) HIP_TRY(hipEventRecord(slot.stamp[5], st));
    return MPC_OK;
}

// ---- the scan route: the seek index's checkpoints found on the device (mp_scan.hip), for a container that comes without an index ----
// mpc::HostStreamScanner's counterpart on a decode slot.  begin() puts the container where upload_and_parse puts it -- at the head of
// the slot's device buffer, through the head of its pinned buffer, zero-padded the same -- so a decode that follows on the same
// slot need not upload it again; behind it the scratch of one window (grow-only, with the slot: 10 bytes per window bit and the
// super-segment maps) and the stream's checkpoints.  scan() hands over to the device once per window and reads 24 bytes back.
struct DeviceStreamScanner : mpc::StreamScanner {
    DecodeSlot& slot;
    const uint8_t* bytes;
    size_t nbytes;
    uint32_t segment_bits, window_bits;
    bool trace;
    mpc_status status = MPC_OK;                 // a HIP failure inside scan(): the caller's status, not a give-up
    int windows = 0, streams = 0;
    float device_ms = 0.f;
    size_t padded = 0;
    mpc::ScanArgs base{};                       // the pointers, and what does not change from window to window
    uint32_t* h_luts = nullptr;                 // pinned: the stream's tables on their way up
    uint32_t* h_lens = nullptr;
    uint16_t* h_tables = nullptr;
    mpc::ScanResult* h_result = nullptr;
    unsigned long long* h_cps = nullptr;
    uint32_t *d_luts = nullptr, *d_lens = nullptr;
    uint16_t* d_tables = nullptr;
    size_t cp_capacity = 0;

    DeviceStreamScanner(DecodeSlot& s, const uint8_t* b, size_t n, uint32_t segment, uint32_t window, bool tr)
        : slot(s), bytes(b), nbytes(n), segment_bits(segment), window_bits(window), trace(tr) {}

    static size_t padded_size(size_t nbytes) { return ((nbytes + 3) & ~static_cast<size_t>(3)) + 16; }

    mpc_status begin(uint32_t interval, bool pooled) {
        constexpr size_t kHead = 256, kLut = size_t(1) << mpc::kParseLutBits;
        const uint64_t total = 8 * static_cast<uint64_t>(nbytes);
        padded = padded_size(nbytes);
        const size_t win = static_cast<size_t>(std::min<uint64_t>(window_bits, std::max<uint64_t>(total, 1)));
        const size_t n_segs = (win + segment_bits - 1) / segment_bits, n_supers = (n_segs + mpc::kScanSuper - 1) / mpc::kScanSuper;
        cp_capacity = static_cast<size_t>(total / interval) + 2;                  // a stream's codes take a bit each at least
        uint8_t* words;
        auto layout = [&](char* b, bool device) {
            Carve cv{b};
            words = cv.take<uint8_t>(padded);
            uint32_t* luts = cv.take<uint32_t>(kLut);
            uint32_t* lens = cv.take<uint32_t>(3 * 33);
            uint16_t* tables = cv.take<uint16_t>(65536);
            unsigned long long* cps = cv.take<unsigned long long>(cp_capacity);
            if (!device) {
                h_luts = luts; h_lens = lens; h_tables = tables; h_cps = cps;
                return cv.at;
            }
            d_luts = luts; d_lens = lens; d_tables = tables;
            base.checkpoints = cps;
            base.step = cv.take<unsigned>(win);
            base.exit_of = cv.take<unsigned>(win);
            base.count = cv.take<uint16_t>(win);
            base.sup_exit = cv.take<unsigned>(n_supers * segment_bits);
            base.sup_count = cv.take<unsigned>(n_supers * segment_bits);
            base.sup_entry = cv.take<unsigned>(n_supers);
            base.sup_ord = cv.take<unsigned long long>(n_supers);
            base.seg_entry = cv.take<unsigned>(n_segs);
            base.seg_ord = cv.take<unsigned long long>(n_segs);
            base.result = cv.take<mpc::ScanResult>(1);
            return cv.at;
        };
        if (const mpc_status gs = slot.pinned.reserve(kHead + layout(nullptr, false), "pinned decode staging"); gs != MPC_OK) return gs;
        if (const mpc_status gs = slot.dev.reserve(layout(nullptr, true), "device decode staging"); gs != MPC_OK) return gs;
        h_result = reinterpret_cast<mpc::ScanResult*>(slot.pinned.data());
        layout(slot.pinned.data() + kHead, false);
        uint8_t* h_words = words;
        layout(slot.dev.data(), true);
        const size_t piece = size_t(1) << 20, pieces = (nbytes + piece - 1) / piece;
        const auto stage = [&](int job) {
            const size_t lo = piece * static_cast<size_t>(job), hi = std::min(nbytes, lo + piece);
            std::memcpy(h_words + lo, bytes + lo, hi - lo);
        };
        if (pooled && pieces > 1) mpc::parallel_jobs(static_cast<int>(pieces), stage);
        else
            for (size_t job = 0; job < pieces; ++job) stage(static_cast<int>(job));
        std::memset(h_words + nbytes, 0, padded - nbytes);
        HIP_TRY(hipMemcpyAsync(words, h_words, padded, hipMemcpyHostToDevice, slot.stream));
        base.tables.words = reinterpret_cast<const uint32_t*>(words);
        base.tables.luts = d_luts;
        base.tables.lens = d_lens;
        base.tables.tables = d_tables;
        base.total_bits = total;
        base.seg_bits = segment_bits;
        base.interval = interval;
        return MPC_OK;
    }

    bool scan(const mpc::StreamWrapper& w, uint64_t b0, uint64_t n, uint32_t interval, std::vector<uint64_t>& cps, uint64_t* end_bit) override {
        status = guarded([&]() -> mpc_status { return scan_stream(w, b0, n, interval, cps, end_bit); });
        return status == MPC_OK && given_up == false;
    }

    bool given_up = false;
    mpc_status scan_stream(const mpc::StreamWrapper& w, uint64_t b0, uint64_t n, uint32_t interval, std::vector<uint64_t>& cps, uint64_t* end_bit) {
        given_up = true;
        const bool golomb = w.mode == 1;
        if (!golomb && w.cb.lut.empty()) return MPC_OK;             // codes longer than 32 bits: serial only
        const uint64_t n_cp = (n + interval - 1) / interval;
        if (n_cp > cp_capacity || interval != base.interval) return MPC_OK;
        hipStream_t st = slot.stream;
        mpc::ScanArgs a = base;
        a.stream = mpc::ParseStream{};
        a.stream.flags = golomb ? mpc::kParseGolomb : 0u;
        a.stream.m = w.m;
        if (!golomb) {                                              // the stream's tables up: the device reads them at offset 0
            std::vector<uint32_t> luts, lens;
            std::vector<uint16_t> tables;
            append_code_tables(w.cb, a.stream, luts, lens, tables);
            std::memcpy(h_luts, luts.data(), sizeof(uint32_t) * luts.size());
            HIP_TRY(hipMemcpyAsync(d_luts, h_luts, sizeof(uint32_t) * luts.size(), hipMemcpyHostToDevice, st));
            if (!lens.empty()) {
                std::memcpy(h_lens, lens.data(), sizeof(uint32_t) * lens.size());
                std::memcpy(h_tables, tables.data(), sizeof(uint16_t) * tables.size());
                HIP_TRY(hipMemcpyAsync(d_lens, h_lens, sizeof(uint32_t) * lens.size(), hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(d_tables, h_tables, sizeof(uint16_t) * tables.size(), hipMemcpyHostToDevice, st));
            }
        }
        a.n = n;
        a.n_cp = n_cp;
        ++streams;
        uint64_t pos = b0, ord = 0;
        for (;;) {                                                  // every window moves pos on by its own length at least, or ends the stream
            if (golomb && ord == n) break;
            if (pos >= base.total_bits) return MPC_OK;
            a.win_begin = pos;
            a.ord0 = ord;
            a.win_bits = static_cast<unsigned>(std::min<uint64_t>(window_bits, base.total_bits - pos));
            a.n_segs = (a.win_bits + segment_bits - 1) / segment_bits;
            a.n_supers = (a.n_segs + mpc::kScanSuper - 1) / mpc::kScanSuper;
            h_result->state = 0;
            if (trace) HIP_TRY(hipEventRecord(slot.stamp[0], st));
            if (const int e = mpc::launch_scan_window(a, st); e != 0) return launch_failed(e);
            if (trace) HIP_TRY(hipEventRecord(slot.stamp[1], st));
            HIP_TRY(hipMemcpyAsync(h_result, a.result, sizeof(mpc::ScanResult), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipEventRecord(slot.done, st));
            HIP_TRY(hipEventSynchronize(slot.done));
            ++windows;
            if (trace) {
                float ms = 0.f;
                (void)hipEventElapsedTime(&ms, slot.stamp[0], slot.stamp[1]);
                device_ms += ms;
            }
            const mpc::ScanResult r = *h_result;
            if (r.state == mpc::kScanEnded) {
                if (r.ordinal != n) return MPC_OK;
                pos = r.position;
                break;
            }
            // the carry: strictly behind the window, or the scan would not end
            if (r.state != mpc::kScanContinue || r.position < pos + a.win_bits || r.position > base.total_bits + mpc::kScanUnaryCap + 64) return MPC_OK;
            pos = r.position;
            ord = r.ordinal;
        }
        if (pos > base.total_bits) return MPC_OK;
        cps.resize(static_cast<size_t>(n_cp));
        if (n_cp) {
            HIP_TRY(hipMemcpyAsync(h_cps, base.checkpoints, sizeof(unsigned long long) * n_cp, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipEventRecord(slot.done, st));
            HIP_TRY(hipEventSynchronize(slot.done));
            std::memcpy(cps.data(), h_cps, sizeof(unsigned long long) * n_cp);
        }
        *end_bit = pos;
        given_up = false;
        return MPC_OK;
    }
};

// The proposal for one container on `slot`: *proposed = false: the scan gave up.  The blob is version 1 and nothing has verified it
mpc_status scan_on_slot(DecodeSlot& slot, const uint8_t* bytes, size_t nbytes, uint32_t interval, uint32_t segment, uint32_t window,
                        bool pooled, bool trace, std::vector<uint8_t>& blob, bool* proposed) {
    *proposed = false;
    if (interval == 0) interval = mpc::kIndexIntervalDefault;
    int width, height, K, block_size;
    if (nbytes == 0 || nbytes > (size_t(1) << 31) || !mpc::container_info(bytes, nbytes, &width, &height, &K, &block_size)) return MPC_OK;
    const double t0 = trace_ms();
    DeviceStreamScanner scanner(slot, bytes, nbytes, segment, window, trace);
    if (const mpc_status bs = scanner.begin(interval, pooled); bs != MPC_OK) return bs;
    *proposed = mpc::propose_container_index(bytes, nbytes, interval, scanner, blob);
    if (scanner.status != MPC_OK) {
        *proposed = false;
        (void)hipStreamSynchronize(slot.stream);
        return scanner.status;
    }
    if (trace)
        std::fprintf(stderr, "[trace] scan: %s after %.2f ms on the host (%d streams, %d windows handed over; their kernels %.2f ms on the device)\n",
                     *proposed ? "proposed" : "gave up", trace_ms() - t0, scanner.streams, scanner.windows, scanner.device_ms);
    return MPC_OK;
}

// Behind upload_and_parse(deferred) for a window of tiles [t0, t1): the lengths stream's parse with hist / verify / void, count and
// scan over all tiles, the ranks of t0 and t1 (d_window, on the device: no round trip), the parse of the window's chunks and the
// unpack of the window's blocks.  sa: block_live and sizes carved, counts and symbols set here.  stamp[6]: behind the ranks,
// [5]: behind the parse, [2]: behind the unpack
// d_span (index version 2, not "parse all"; the upload was made with_aux): packed and step-0 coefficient streams are cut as well, by
// mp_window_rank_kernel<true> and launch_unpack_window_cut; null: the launches of a version-1 index.  ranks_only: nothing behind
// the rank kernel is launched (mpc_window_chunks_device).  clamp_steps (a view; pp planned with the same keep_steps): the lengths
// are cut to it between their check and the ranks
mpc_status parse_and_unpack_window(DecodeSlot& slot, UnpackJob& j, const ParsePlan& pp, mpc::ParseArgs pa, mpc::StreamArgs& sa,
                                   mpc::WindowStream* d_window, const mpc::TileWindow& win, bool parse_all, mpc::WindowSpan* d_span = nullptr,
                                   bool ranks_only = false, int clamp_steps = 0) {
    hipStream_t st = slot.stream;
    sa.counts = pa.counts;
    sa.symbols = j.ua.symbols;
    pa.window = d_window;
    pa.group_first = pp.streams[1].group_begin;                     // the lengths stream's groups come first
    if (const int e = mpc::launch_parse_lengths(pa, st); e != 0) return launch_failed(e);
    if (clamp_steps)
        if (const int e = mpc::launch_clamp_lengths(pa, clamp_steps, st); e != 0) return launch_failed(e);
    mpc::WindowArgs wa{};
    wa.sa = sa;
    wa.unpack = j.ua.streams;
    wa.parse = pa.streams;
    wa.interval = pa.interval;
    wa.parse_all = parse_all ? 1 : 0;
    wa.t0 = static_cast<long long>(win.t0);
    wa.t1 = static_cast<long long>(win.t1);
    wa.window = d_window;
    if (d_span) {
        wa.aux = j.d_aux;
        wa.aux_off = j.d_aux_off;
        wa.span = d_span;
    }
    if (const int e = mpc::launch_window_rank(wa, st); e != 0) return launch_failed(e);
    if (j.trace) HIP_TRY(hipEventRecord(slot.stamp[6], st));
    if (ranks_only) return MPC_OK;
    if (const int e = mpc::launch_parse_window(pa, st); e != 0) return launch_failed(e);
    if (j.trace) HIP_TRY(hipEventRecord(slot.stamp[5], st));
    j.ua.window = d_window;
    if (d_span) {
        if (const int e = mpc::launch_unpack_window_cut(mpc::UnpackWindowArgs{j.ua, d_span}, st); e != 0) return launch_failed(e);
    } else if (const int e = mpc::launch_unpack_window(j.ua, st); e != 0)
        return launch_failed(e);
    if (j.trace) HIP_TRY(hipEventRecord(slot.stamp[2], st));
    return MPC_OK;
}

// what frame_on_slot needs of a frame's header, whichever route parsed it
struct FrameHead {
    int width = 0, height = 0, K = 0;
    size_t n_tc = 0;                            // 3 * tiles
    const uint16_t (*quant)[32] = nullptr;
};

// What the container parts of a compose (include/mpcodec.h, "compose") write into: the call's destination records in whole-frame
// layout and its owner map, in device memory; frame f of the sequence is part part_of_frame[f] of the call
struct ComposeTarget {
    uint16_t* d_counts = nullptr;
    uint32_t* d_choices = nullptr;
    const int32_t* d_owner = nullptr;
    int tiles_x = 0, tiles_y = 0;
    const int* part_of_frame = nullptr;
    const mpc::ComposePart* parts = nullptr;
};

// A compose's container part behind the gather, the third mode beside the reconstruction and transcode_on_slot: the paste kernel moves
// the rectangle's records from the slot's (frame layout, `counts` / `choices`) straight into the tiles of the call's destination that
// the part owns.  It writes nothing but those tiles, whatever the records hold, and the slot's error words are read before the frame
// counts: a part the index route refuses starts over on the serial route and writes the same tiles again.  *refused as in frame_on_slot
mpc_status paste_on_slot(Sequence& q, int f, DecodeSlot& slot, UnpackJob& j, const uint16_t* counts, const uint32_t* choices, int width, int K,
                         const mpc::TileWindow& win, bool indexed, double stamps[3], bool* refused) {
    const ComposeTarget& to = *q.compose;
    hipStream_t st = slot.stream;
    const int part = to.part_of_frame[f], bs = q.c->block_size;
    const mpc::ComposePart& piece = to.parts[part];
    // the reconstruction's error word is this route's "a count above K", as for a transcode
    if (const int e = mpc::launch_paste_records(counts, choices, (width + bs - 1) / bs, win.tiles_y, win.tx0, win.ty0, win.tx1 - win.tx0,
                                                win.ty1 - win.ty0, K, to.d_counts, to.d_choices, to.tiles_x, to.tiles_y, piece.dx / bs,
                                                piece.dy / bs, to.d_owner, part, j.ua.error + 1, st);
        e != 0)
        return launch_failed(e);
    if (q.tuning.trace) HIP_TRY(hipEventRecord(slot.stamp[3], st));
    HIP_TRY(hipMemcpyAsync(j.h_flags, j.ua.error, 3 * sizeof(int), hipMemcpyDeviceToHost, st));
    if (q.tuning.trace) HIP_TRY(hipEventRecord(slot.stamp[4], st));
    HIP_TRY(hipEventRecord(slot.done, st));
    HIP_TRY(hipEventSynchronize(slot.done));                        // the paste has finished: the call waits for every part's
    stamps[1] = trace_ms();
    if (indexed && (j.h_flags[2] != 0 || j.h_flags[0] != 0)) {
        *refused = true;
        return MPC_OK;
    }
    if (j.h_flags[0] != 0) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
    if (j.h_flags[1] != 0) return fail(MPC_ERR_BITSTREAM, "Invalid bitstream");
    q.width[f] = q.rects[f].width;
    q.height[f] = q.rects[f].height;
    stamps[2] = trace_ms();
    return MPC_OK;
}

// A transcode's frame behind the gather, in place of the reconstruction: the crop kernel moves the rectangle's records (frame layout,
// `counts` / `choices`) into the new frame's tile order, cut to `steps`, and the records-to-container chain (ContainerJob) codes them
// on the job slot of this decode slot's number, on the slot's own stream.  The error words are read first: records the index route
// is about to refuse, or a count above K, never enter the chain.  *refused as in frame_on_slot
mpc_status transcode_on_slot(Sequence& q, int f, DecodeSlot& slot, UnpackJob& j, const uint16_t* counts, const uint32_t* choices, int width,
                             int height, int K, const mpc::TileWindow& win, int steps, const double* quant, uint16_t* d_crop_counts,
                             uint32_t* d_crop_choices, bool indexed, double stamps[3], bool* refused) {
    mpc_context* c = q.c;
    hipStream_t st = slot.stream;
    const mpc_rect& rc = q.rects[f];
    const int bs = c->block_size, tiles_x = (width + bs - 1) / bs;
    // the reconstruction's error word is this route's "a count above K": the same verdict, "Invalid bitstream"
    if (const int e = mpc::launch_crop_records(counts, choices, tiles_x, win.tiles_y, win.tx0, win.ty0, win.tx1, win.ty1, K, steps, d_crop_counts,
                                               d_crop_choices, j.ua.error + 1, st);
        e != 0)
        return launch_failed(e);
    if (q.tuning.trace) HIP_TRY(hipEventRecord(slot.stamp[3], st));
    HIP_TRY(hipMemcpyAsync(j.h_flags, j.ua.error, 3 * sizeof(int), hipMemcpyDeviceToHost, st));
    if (q.tuning.trace) HIP_TRY(hipEventRecord(slot.stamp[4], st));
    HIP_TRY(hipEventRecord(slot.done, st));
    HIP_TRY(hipEventSynchronize(slot.done));
    stamps[1] = trace_ms();
    if (indexed && (j.h_flags[2] != 0 || j.h_flags[0] != 0)) {
        *refused = true;
        return MPC_OK;
    }
    if (j.h_flags[0] != 0) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
    if (j.h_flags[1] != 0) return fail(MPC_ERR_BITSTREAM, "Invalid bitstream");
    JobSlot& js = *c->jobs[static_cast<size_t>(f % q.slots)];      // created, and found idle, by the call
    const long long tiles = static_cast<long long>(win.tx1 - win.tx0) * (win.ty1 - win.ty0);
    Carve measure;
    mpc::StreamArgs measured{};
    carve_stream_buffers(measure, tiles, K, true, &measured);
    if (const mpc_status gs = js.dev.reserve(measure.at, "device staging"); gs != MPC_OK) return gs;
    GrowBuffer host_stage(GrowBuffer::kPinned);                     // the host route's, should the frame take it: this frame's own
    ContainerJob& job = js.job;
    job.side = job.down = st;
    job.spin = q.n == 1;
    job.host_stage = &host_stage;
    job.host_offset = 0;
    job.index_interval = 0;
    job.index_expanded = false;
    struct Unhook {
        ContainerJob& job;
        ~Unhook() { job.host_stage = nullptr; }
    } unhook{job};
    EntropyBuffers eb;
    if (!q.tuning.host_entropy)
        if (const mpc_status es = entropy_buffers(js.ent, static_cast<size_t>(tiles), K, &eb); es != MPC_OK) return es;
    HIP_TRY(hipStreamSynchronize(nullptr));                         // a slot carved for another geometry clears its tables on the null stream
    if (const mpc_status bs_ = container_begin(job, c, q.tuning.host_entropy ? nullptr : &eb, q.tuning.triple_limit, js.dev.data(), d_crop_counts,
                                               d_crop_choices, nullptr, nullptr, rc.width, rc.height, quant);
        bs_ != MPC_OK)
        return bs_;
    if (const mpc_status ts = container_tables(job); ts != MPC_OK) return ts;
    uint8_t* made = nullptr;
    size_t made_bytes = 0;
    if (const mpc_status cs = container_collect(job, &made, &made_bytes); cs != MPC_OK) return cs;
    HIP_TRY(hipStreamSynchronize(st));                              // the job's buffers are the next frame's
    q.containers[f] = made;
    q.container_bytes[f] = made_bytes;
    q.width[f] = rc.width;
    q.height[f] = rc.height;
    stamps[2] = trace_ms();
    return MPC_OK;
}

// upload | (parse) | unpack | gather | reconstruct | (host form) pixels down, on the slot's stream; returns with the frame complete.
// s: the serially parsed streams, or pp: the checked index (then *refused = true with MPC_OK says that the device's half of the
// acceptance rule failed: nothing of the frame counts, the serial route starts over)
mpc_status frame_on_slot(Sequence& q, int f, DecodeSlot& slot, const FrameHead& s, const UnpackPlan& plan, const mpc::CodedStreams* serial,
                         const ParsePlan* pp, double stamps[3], bool* refused, bool words_resident = false) {
    mpc_context* c = q.c;
    const bool trace = q.tuning.trace;
    const int K = s.K;
    const size_t n_tc = s.n_tc, tiles = n_tc / 3;
    const size_t px = static_cast<size_t>(s.width) * s.height * 3;
    // A rectangle of the frame: with a checked index the window alone (`windowed`), else the whole frame into the slot's own memory
    // and a 2-D copy (`crop`).  The call has checked the rectangle against the container's header; this is the frame's own.
    const mpc_rect* rc = q.rects ? &q.rects[f] : nullptr;
    mpc::TileWindow win;
    if (rc && !mpc::tile_window(s.width, s.height, c->block_size, rc->x, rc->y, rc->width, rc->height, win))
        return fail(MPC_ERR_ARGUMENT, "rectangle %dx%d at (%d, %d) in a frame of %dx%d", rc->width, rc->height, rc->x, rc->y, s.width, s.height);
    // A view: the region's window route, or the whole frame's streams by the serial route (parse_worker has cut them), and either way
    // mp_decode_view_kernel on the rectangle's tiles: no full-size frame, no 2-D copy
    const mpc_view* vw = q.views ? &q.views[f] : nullptr;
    const bool windowed = rc && pp, crop = rc && !pp && !vw;
    const bool cut = windowed && pp->expanded && !q.parse_all;      // index version 2: packed and step-0 streams through their aux entries
    const size_t out_px = q.out_bytes(f, s.width, s.height);
    // read_compressed_coded refuses any other K; `quant` and UnpackJob::streams are sized by MPC_MAX_K and must not lean on that
    if (K < 1 || K > MPC_MAX_K) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
    const mpc::DecodeView dv{vw ? view_steps(vw->steps, K) : K, vw ? vw->scale_log2 : 0};
    // pp was planned with the same steps (parse_worker); "parse all" parses, unpacks and gathers every stream, the kernel alone cuts
    const int clamp_steps = vw && windowed && !q.parse_all && dv.steps < K ? dv.steps : 0;
    double quant[3 * MPC_MAX_K];
    for (int ch = 0; ch < 3; ++ch)
        for (int i = 0; i < K; ++i) quant[ch * K + i] = static_cast<double>(s.quant[ch][i]);
    mpc::StreamArgs sa{};
    uint32_t* d_choices;
    uint8_t *d_pixels = nullptr, *d_full = nullptr;
    mpc::WindowStream* d_window = nullptr;
    mpc::WindowSpan* d_span = nullptr;
    uint16_t* d_crop_counts = nullptr;                              // a transcode: the rectangle's tiles as a frame of their own
    uint32_t* d_crop_choices = nullptr;
    const size_t crop_tc = q.containers ? 3 * static_cast<size_t>(win.tx1 - win.tx0) * static_cast<size_t>(win.ty1 - win.ty0) : 0;
    auto behind_layout = [&](char* base) {                          // behind the unpacked streams: records | the gather's scratch | pixels
        Carve cv{base};
        d_choices = cv.take<uint32_t>(n_tc * K);
        carve_stream_buffers(cv, static_cast<long long>(tiles), K, false, &sa);
        if (windowed) d_window = cv.take<mpc::WindowStream>(6 * static_cast<size_t>(K));
        if (cut) d_span = cv.take<mpc::WindowSpan>(6 * static_cast<size_t>(K));
        if (q.containers) {
            d_crop_counts = cv.take<uint16_t>(crop_tc + 2);
            d_crop_choices = cv.take<uint32_t>(crop_tc * K);
        } else if (crop) d_full = cv.take<uint8_t>(px);             // the whole frame, of which the rectangle is copied out
        else if (!q.d_rgb) d_pixels = cv.take<uint8_t>(out_px);
        return cv.at;
    };
    UnpackJob j;
    j.plan = &plan;
    j.K = K;
    if (serial) {
        for (int i = 0; i < 6 * K; ++i) j.streams[i] = serial->codes[i].data();
        j.extra[0] = serial->lengths.data();
        j.extra_bytes[0] = sizeof(uint16_t) * n_tc;
    }
    j.extra[1] = quant;
    j.extra_bytes[1] = sizeof(double) * 3 * static_cast<size_t>(K);
    j.behind_bytes = behind_layout(nullptr);
    j.result_bytes = q.d_rgb ? 0 : out_px;
    // A call of one frame has no other frame's thread to share the cores with: its copies go through the worker pool.  Otherwise
    // every frame's thread copies its own.
    const bool pooled = q.n == 1;
    j.pooled = pooled;
    j.trace = trace;
    hipStream_t st = slot.stream;
    if (serial) {
        if (const mpc_status us = upload_and_unpack(slot, j); us != MPC_OK) return us;
    } else if (!windowed) {
        if (const mpc_status us = upload_and_parse(slot, j, *pp, q.bytes[f], q.nbytes[f], nullptr, false, words_resident); us != MPC_OK) return us;
        if (const int e = mpc::launch_unpack(j.ua, st); e != 0) return launch_failed(e);
        if (trace) HIP_TRY(hipEventRecord(slot.stamp[2], st));
    } else {
        mpc::ParseArgs pa{};
        if (const mpc_status us = upload_and_parse(slot, j, *pp, q.bytes[f], q.nbytes[f], &pa, cut); us != MPC_OK) return us;
        behind_layout(j.d_behind);
        if (const mpc_status ws = parse_and_unpack_window(slot, j, *pp, pa, sa, d_window, win, q.parse_all, d_span, false, clamp_steps); ws != MPC_OK)
            return ws;
    }
    stamps[0] = j.staged_ms;
    const uint16_t* counts = static_cast<const uint16_t*>(j.d_extra[0]);
    behind_layout(j.d_behind);
    if (q.d_rgb && !crop) d_pixels = q.d_rgb[f];
    sa.counts = counts;
    sa.symbols = j.ua.symbols;
    mpc::DecodeWindow dw{};
    if (rc) dw = mpc::DecodeWindow{rc->x, rc->y, rc->width, rc->height, win.tx0, win.ty0, win.tx1, win.ty1};
    if (windowed) {
        if (const int e = mpc::launch_stream_gather_window(sa, d_choices, static_cast<long long>(win.t0), static_cast<long long>(win.t1), st); e != 0)
            return launch_failed(e);
    } else if (const int e = mpc::launch_stream_gather(sa, d_choices, st); e != 0)
        return launch_failed(e);
    if (q.compose) return paste_on_slot(q, f, slot, j, counts, d_choices, s.width, K, win, pp != nullptr, stamps, refused);
    if (q.containers)
        return transcode_on_slot(q, f, slot, j, counts, d_choices, s.width, s.height, K, win, dv.steps, quant, d_crop_counts, d_crop_choices,
                                 pp != nullptr, stamps, refused);
    if (const mpc_status ds = decode_tiles_on_device(c, counts, d_choices, static_cast<const double*>(j.d_extra[1]), K, s.width, s.height,
                                                     crop ? d_full : d_pixels, j.ua.error + 1, st, windowed || vw ? &dw : nullptr,
                                                     vw ? &dv : nullptr);
        ds != MPC_OK)
        return ds;
    if (trace) HIP_TRY(hipEventRecord(slot.stamp[3], st));
    HIP_TRY(hipMemcpyAsync(j.h_flags, j.ua.error, 3 * sizeof(int), hipMemcpyDeviceToHost, st));
    if (crop) {                                                     // rows of the rectangle out of the whole frame's
        const size_t row = 3 * static_cast<size_t>(rc->width), pitch = 3 * static_cast<size_t>(s.width);
        const uint8_t* from = d_full + 3 * (static_cast<size_t>(rc->y) * s.width + rc->x);
        HIP_TRY(hipMemcpy2DAsync(q.d_rgb ? static_cast<void*>(q.d_rgb[f]) : static_cast<void*>(j.h_result), row, from, pitch, row,
                                 static_cast<size_t>(rc->height), q.d_rgb ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    } else if (!q.d_rgb)
        HIP_TRY(hipMemcpyAsync(j.h_result, d_pixels, out_px, hipMemcpyDeviceToHost, st));          // the upload has left the buffer: stream order
    if (trace) HIP_TRY(hipEventRecord(slot.stamp[4], st));
    HIP_TRY(hipEventRecord(slot.done, st));
    HIP_TRY(hipEventSynchronize(slot.done));                        // this frame's work only: no other context's, no other slot's
    stamps[1] = trace_ms();
    // a chunk, a length or a stream size is not what the index says; for a window also a packed stream that does not expand to its
    // size: not every chunk in front of it need have been parsed, so that verdict is the serial route's to give
    if (pp && (j.h_flags[2] != 0 || (windowed && j.h_flags[0] != 0))) {
        *refused = true;                                            // (the caller passes `refused` whenever it passes `pp`)
        return MPC_OK;
    }
    // a stream that does not expand to its size is what mpc::read_compressed refuses, a record outside its dictionary the reconstruction
    if (j.h_flags[0] != 0) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
    if (j.h_flags[1] != 0) return fail(MPC_ERR_BITSTREAM, "Invalid bitstream");
    if (!q.d_rgb) {
        uint8_t* out = static_cast<uint8_t*>(std::malloc(out_px ? out_px : 1));
        if (!out) return fail(MPC_ERR_ALLOC, "out of memory");
        // a few threads fault the caller's fresh pages in and copy
        const size_t piece = pooled ? ((out_px + 15) / 16 + 4095) & ~static_cast<size_t>(4095) : out_px;
        const auto copy = [&](int k) {
            const size_t lo = piece * static_cast<size_t>(k), hi = std::min(out_px, lo + piece);
            std::memcpy(out + lo, j.h_result + lo, hi - lo);
        };
        if (pooled && out_px) mpc::parallel_jobs(static_cast<int>((out_px + piece - 1) / piece), copy);
        else if (out_px) copy(0);                                       // the frames' copies run side by side on the call's threads
        q.rgb[f] = out;
    }
    q.width[f] = vw ? view_extent(rc->width, vw->scale_log2) : s.width;
    q.height[f] = vw ? view_extent(rc->height, vw->scale_log2) : s.height;
    stamps[2] = trace_ms();
    return MPC_OK;
}

void trace_frame(int f, int slot_index, DecodeSlot& slot, const double host[6], bool indexed, bool windowed) {
    float dev[4] = {};
    for (int k = 0; k < 4; ++k) (void)hipEventElapsedTime(&dev[k], slot.stamp[k], slot.stamp[k + 1]);
    if (windowed) {
        float lengths = 0.f, parse = 0.f, unpack = 0.f;
        (void)hipEventElapsedTime(&lengths, slot.stamp[1], slot.stamp[6]);
        (void)hipEventElapsedTime(&parse, slot.stamp[6], slot.stamp[5]);
        (void)hipEventElapsedTime(&unpack, slot.stamp[5], slot.stamp[2]);
        std::fprintf(stderr,
                     "[trace] decode frame %d slot %d, route window: parse: tables %.2f ms | wait for the slot %.2f | staged %.2f | on the "
                     "device %.2f (upload %.2f, lengths parse + ranks %.2f, windowed parse %.2f, unpack %.2f, gather + reconstruct %.2f, "
                     "copy-out %.2f) | pixels to the caller %.2f\n",
                     f, slot_index, host[1] - host[0], host[2] - host[1], host[3] - host[2], host[4] - host[3], dev[0], lengths, parse, unpack,
                     dev[2], dev[3], host[5] - host[4]);
        return;
    }
    if (indexed) {
        float parse = 0.f, unpack = 0.f;
        (void)hipEventElapsedTime(&parse, slot.stamp[1], slot.stamp[5]);
        (void)hipEventElapsedTime(&unpack, slot.stamp[5], slot.stamp[2]);
        std::fprintf(stderr,
                     "[trace] decode frame %d slot %d, route device: parse: tables %.2f ms, kernels %.2f | wait for the slot %.2f | staged %.2f | "
                     "on the device %.2f (upload %.2f, parse %.2f, unpack %.2f, gather + reconstruct %.2f, copy-out %.2f) | pixels to the "
                     "caller %.2f\n",
                     f, slot_index, host[1] - host[0], parse, host[2] - host[1], host[3] - host[2], host[4] - host[3], dev[0], parse, unpack,
                     dev[2], dev[3], host[5] - host[4]);
        return;
    }
    std::fprintf(stderr,
                 "[trace] decode frame %d slot %d, route serial: parse %.2f ms | wait for the slot %.2f | staged %.2f | on the device %.2f (upload %.2f, "
                 "unpack %.2f, gather + reconstruct %.2f, copy-out %.2f) | pixels to the caller %.2f\n",
                 f, slot_index, host[1] - host[0], host[2] - host[1], host[3] - host[2], host[4] - host[3], dev[0], dev[1], dev[2], dev[3],
                 host[5] - host[4]);
}

void parse_worker(Sequence& q) {
    mpc_context* c = q.c;
    for (;;) {
        const int f = q.next.fetch_add(1);
        if (f >= q.n) return;
        double host[6] = {};
        host[0] = trace_ms();
        mpc::CodedStreams s;
        UnpackPlan plan;
        ParsePlan pp;
        FrameHead head;
        // the serial route's parse: what the format chains from code to code, on this thread
        const auto parse_serial = [&]() -> mpc_status {
            if (q.failed_before(f)) return MPC_OK;
            HIP_TRY(hipSetDevice(c->device));
            if (!mpc::read_compressed_coded(q.bytes[f], q.nbytes[f], s)) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
            const bool block_size_differs = s.block_size != c->block_size;
            // a view of the first `steps` steps decodes the truncated container: its lengths are min(length, steps)
            const int steps = q.views && q.views[f].steps > 0 ? q.views[f].steps : INT_MAX;
            // (a transcode refuses a length above K wherever it is cut to, as mpc_transcode_container does, and a K that is not the context's)
            const int held = q.containers || q.compose ? INT_MAX : steps;
            const bool too_long = std::any_of(s.lengths.begin(), s.lengths.end(), [&](uint16_t length) { return std::min<int>(length, held) > s.K; });
            const bool K_differs = q.containers && s.K != c->K;
            if (block_size_differs || K_differs || too_long) {
                // Refused here, before the device has expanded a stream.  A container whose streams do not expand either is
                // invalid data first, whatever else is wrong with it: the host's expansion (the reference for what a decoder
                // accepts) gives that verdict, on this path alone.
                mpc::Streams expanded;
                if (!mpc::read_compressed(q.bytes[f], q.nbytes[f], expanded)) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
                if (block_size_differs)
                    return fail(MPC_ERR_ARGUMENT, "stream block size %d, context block size %d", s.block_size, c->block_size);
                if (K_differs) return fail(MPC_ERR_ARGUMENT, "container K %d, context K %d", s.K, c->K);
                return fail(MPC_ERR_BITSTREAM, "Invalid bitstream");
            }
            if (q.d_rgb && !q.rects && q.out_bytes(f, s.width, s.height) > q.capacity[f])
                return fail(MPC_ERR_ARGUMENT, "capacity %zu for a frame of %dx%d", q.capacity[f], s.width, s.height);
            if (steps < s.K) {
                // The truncation's cut (mpc::truncate_container) on the coded streams: a stream of a step at or above `steps` is held
                // to the size the lengths give it, as read_compressed holds it, and emptied; the device sees nothing of it
                for (int i = 0; i < 6 * s.K; ++i) {
                    if ((i % (2 * s.K)) / 2 < steps) continue;
                    std::vector<uint16_t>& v = s.codes[static_cast<size_t>(i)];
                    size_t expanded = v.size();
                    if (s.packed[static_cast<size_t>(i)] && !mpc::rle_decoded_size(v.data(), v.size(), s.expect[static_cast<size_t>(i)], &expanded))
                        return fail(MPC_ERR_BITSTREAM, "Invalid input data");
                    if (expanded != s.expect[static_cast<size_t>(i)]) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
                    v.clear();
                    s.packed[static_cast<size_t>(i)] = 0;
                    s.expect[static_cast<size_t>(i)] = 0;
                }
                for (uint16_t& length : s.lengths) length = std::min<uint16_t>(length, static_cast<uint16_t>(steps));
            }
            if (!plan_unpack(s.K, [&](int i) { return static_cast<unsigned long long>(s.codes[i].size()); }, s.packed.data(), nullptr,
                             s.expect.data(), plan))
                return fail(MPC_ERR_BITSTREAM, "Invalid bitstream");
            head.width = s.width;
            head.height = s.height;
            head.K = s.K;
            head.n_tc = s.lengths.size();
            head.quant = s.quant;
            return MPC_OK;
        };
        // The indexed route's share of the host: the index checked against the container, the code tables built.  It refuses nothing
        // itself: whatever it cannot take, the serial route decides.
        bool indexed = false;
        // The scan route: the frame takes its slot first (in frame order, as below), puts the container on it and has the device find
        // the checkpoints; what it proposes is then this frame's index, checked like any other.  It refuses nothing either
        const int slot_index = f % q.slots;
        const auto take_slot = [&] {
            std::unique_lock<std::mutex> hold(q.lock);
            q.turn.wait(hold, [&] { return q.slot_uses[slot_index] == f / q.slots; });
        };
        std::vector<uint8_t> scanned;
        bool proposed = false;
        mpc_status st = MPC_OK;
        if (q.scan) {
            take_slot();
            if (!q.failed_before(f))
                st = guarded([&]() -> mpc_status {
                    HIP_TRY(hipSetDevice(c->device));
                    return scan_on_slot(*c->dec[slot_index], q.bytes[f], q.nbytes[f], 0, mpc::kScanSegmentDefault, mpc::kScanWindowDefault, q.n == 1,
                                        q.tuning.trace, scanned, &proposed);
                });
        }
        const uint8_t* const index = q.scan ? (proposed ? scanned.data() : nullptr) : q.indexes ? q.indexes[f] : nullptr;
        const size_t index_size = q.scan ? scanned.size() : index ? q.index_bytes[f] : 0;
        if (st == MPC_OK) st = guarded([&]() -> mpc_status {
            if (index && !q.failed_before(f)) {
                HIP_TRY(hipSetDevice(c->device));
                const mpc::ContainerIndex& x = pp.ip.index;
                indexed = plan_parse(q.bytes[f], q.nbytes[f], index, index_size, q.n == 1, pp,
                                     q.views && !q.parse_all ? q.views[f].steps : 0) &&
                          x.block_size == c->block_size && !(q.containers && x.K != c->K) &&
                          !(q.d_rgb && q.out_bytes(f, x.width, x.height) > q.capacity[f]);
                if (indexed) {
                    head.width = x.width;
                    head.height = x.height;
                    head.K = x.K;
                    head.n_tc = pp.n_counts;
                    head.quant = pp.ip.quant;
                    return MPC_OK;
                }
            }
            return parse_serial();
        });
        host[1] = trace_ms();
        // The slot is taken in frame order whatever became of the parse: the frames behind count this slot's uses.
        if (!q.scan) take_slot();
        host[2] = trace_ms();
        bool ran = false;
        if (st == MPC_OK && !q.failed_before(f)) {
            DecodeSlot& slot = *c->dec[slot_index];
            bool refused = false, decoded = true;
            st = guarded([&]() -> mpc_status {
                return frame_on_slot(q, f, slot, head, indexed ? pp.unpack : plan, indexed ? nullptr : &s, indexed ? &pp : nullptr, host + 3, &refused,
                                     q.scan && proposed);
            });
            if (st == MPC_OK && refused) {                          // the serial route from the start, on the slot this frame holds
                indexed = false;
                host[0] = trace_ms();
                st = guarded(parse_serial);
                host[1] = host[2] = trace_ms();
                decoded = st == MPC_OK && !q.failed_before(f);      // parse_serial parses nothing once a frame in front has failed
                if (decoded) st = guarded([&]() -> mpc_status { return frame_on_slot(q, f, slot, head, plan, &s, nullptr, host + 3, nullptr); });
            }
            ran = st == MPC_OK && decoded;
            if (st != MPC_OK) (void)hipStreamSynchronize(slot.stream);             // nothing of this frame is left on the slot's stream
        }
        if (ran && q.routes) q.routes[f] = indexed ? 0 : 1;
        if (ran && indexed && q.out_indexes) {                      // the device has accepted it: the serial builder's blob, for a cache
            uint8_t* copy = static_cast<uint8_t*>(std::malloc(scanned.size()));
            if (!copy) st = fail(MPC_ERR_ALLOC, "out of memory");
            else {
                std::memcpy(copy, scanned.data(), scanned.size());
                q.out_indexes[f] = copy;
                q.out_index_bytes[f] = scanned.size();
            }
        }
        if (ran && q.tuning.trace) trace_frame(f, slot_index, *c->dec[slot_index], host, indexed, indexed && q.rects);
        {
            std::lock_guard<std::mutex> hold(q.lock);
            ++q.slot_uses[slot_index];
        }
        q.turn.notify_all();
        if (st != MPC_OK) q.record_failure(f, st);
    }
}

mpc_status ensure_slots(mpc_context* c, int slots) {
    for (int k = 0; k < slots; ++k) {
        if (c->dec[k]) continue;
        std::unique_ptr<DecodeSlot> d(new DecodeSlot);
        HIP_TRY(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&d->done, hipEventBlockingSync));     // the parse threads sleep on it: their cores parse
        for (hipEvent_t& e : d->stamp) HIP_TRY(hipEventCreate(&e));
        c->dec[k] = std::move(d);
    }
    return MPC_OK;
}

// single: the call is mpc_decode_image's; its error text names no frame
mpc_status decode_sequence(mpc_context* c, const uint8_t* const* bytes, const size_t* nbytes, int n_frames, uint8_t** rgb,
                           uint8_t* const* d_rgb, const size_t* capacity, int* width, int* height, bool single = false,
                           const uint8_t* const* indexes = nullptr, const size_t* index_bytes = nullptr, int* routes = nullptr,
                           const mpc_rect* rects = nullptr, unsigned region_flags = 0, const mpc_view* views = nullptr, bool scan = false,
                           uint8_t** out_indexes = nullptr, size_t* out_index_bytes = nullptr, uint8_t** containers = nullptr,
                           size_t* container_bytes = nullptr, const ComposeTarget* compose = nullptr) {
    // containers (with views and their rectangles): a transcode; no pixels in either form.  compose (likewise): the container parts of
    // a compose, whose error texts name the part
    if (indexes && !index_bytes) return fail(MPC_ERR_ARGUMENT, "null argument");
    if (containers && (!container_bytes || !views || rgb || d_rgb)) return fail(MPC_ERR_ARGUMENT, "null argument");
    if (out_indexes && !out_index_bytes) return fail(MPC_ERR_ARGUMENT, "null argument");
    if (compose && (!views || rgb || d_rgb || containers)) return fail(MPC_ERR_ARGUMENT, "null argument");
    if (!c || !bytes || !nbytes || !width || !height || (!rgb && !d_rgb && !containers && !compose) || (d_rgb && !capacity))
        return fail(MPC_ERR_ARGUMENT, "null argument");
    if (n_frames < 1) return fail(MPC_ERR_ARGUMENT, "n_frames must be at least 1");
    if (c->device < 0) return no_device();
    for (int f = 0; f < n_frames; ++f)
        if (!bytes[f] || (d_rgb && !d_rgb[f])) return fail(MPC_ERR_ARGUMENT, "frame %d: null argument", f);
    if (rects)                                                      // the same for rectangles: the container's own width and height
        for (int f = 0; f < n_frames; ++f) {
            const mpc_rect& r = rects[f];
            if (r.width < 1 || r.height < 1) return fail(MPC_ERR_ARGUMENT, "frame %d: rectangle %dx%d is empty", f, r.width, r.height);
            int w, h, K, bs;
            mpc::TileWindow win;
            if (mpc::container_info(bytes[f], nbytes[f], &w, &h, &K, &bs) && !mpc::tile_window(w, h, bs, r.x, r.y, r.width, r.height, win))
                return fail(MPC_ERR_ARGUMENT, "frame %d: rectangle %dx%d at (%d, %d) is not inside a frame of %dx%d", f, r.width, r.height, r.x,
                            r.y, w, h);
            if (views) {
                const int vw = view_extent(r.width, views[f].scale_log2), vh = view_extent(r.height, views[f].scale_log2);
                if (d_rgb && static_cast<size_t>(vw) * static_cast<size_t>(vh) * 3 > capacity[f])
                    return fail(MPC_ERR_ARGUMENT, "frame %d: capacity %zu for a view of %dx%d", f, capacity[f], vw, vh);
            } else if (d_rgb && static_cast<size_t>(r.width) * static_cast<size_t>(r.height) * 3 > capacity[f])
                return fail(MPC_ERR_ARGUMENT, "frame %d: capacity %zu for a rectangle of %dx%d", f, capacity[f], r.width, r.height);
        }
    else if (d_rgb)                                                 // before anything is enqueued; a header that does not parse fails in its turn
        for (int f = 0; f < n_frames; ++f) {
            int w, h, K, bs;
            if (mpc::container_info(bytes[f], nbytes[f], &w, &h, &K, &bs) && static_cast<size_t>(w) * h * 3 > capacity[f])
                return fail(MPC_ERR_ARGUMENT, "frame %d: capacity %zu for a frame of %dx%d", f, capacity[f], w, h);
        }
    std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
    HIP_TRY(hipSetDevice(c->device));
    Sequence q;
    q.c = c;
    q.tuning = read_tuning();
    q.n = n_frames;
    q.single = single;
    q.slots = mpc_context::kDecodeSlots;
    q.bytes = bytes;
    q.nbytes = nbytes;
    q.rgb = rgb;
    q.d_rgb = d_rgb;
    q.capacity = capacity;
    q.indexes = indexes;
    q.index_bytes = index_bytes;
    q.routes = routes;
    q.rects = rects;
    q.parse_all = (region_flags & MPC_REGION_PARSE_ALL) != 0;
    q.views = views;
    q.scan = scan;
    q.out_indexes = out_indexes;
    q.out_index_bytes = out_index_bytes;
    if (out_indexes) {
        std::fill(out_indexes, out_indexes + n_frames, nullptr);
        std::fill(out_index_bytes, out_index_bytes + n_frames, 0);
    }
    if (routes) std::fill(routes, routes + n_frames, 1);
    q.width = width;
    q.height = height;
    if (const mpc_status ss = ensure_slots(c, q.slots); ss != MPC_OK) return ss;
    if (containers) {
        // frame f codes its container on job slot f % slots, its own for as long as it holds the decode slot of that number
        static_assert(mpc_context::kSeqSlots >= mpc_context::kDecodeSlots, "a container job slot per decode slot");
        for (int k = 0; k < mpc_context::kSeqSlots; ++k)
            if (c->jobs[k] && c->jobs[k]->stage != 0) return fail(MPC_ERR_ARGUMENT, "container job slot %d is busy", k);
        for (int k = 0; k < q.slots; ++k) {
            if (!c->jobs[k]) c->jobs[k] = std::make_unique<JobSlot>();
            ContainerJob& job = c->jobs[k]->job;
            if (!job.phase1) {
                HIP_TRY(hipEventCreateWithFlags(&job.phase1, hipEventDisableTiming | hipEventBlockingSync));
                HIP_TRY(hipEventCreateWithFlags(&job.done, hipEventDisableTiming | hipEventBlockingSync));
            }
        }
        q.containers = containers;
        q.container_bytes = container_bytes;
    }
    q.compose = compose;
    if (rgb) std::fill(rgb, rgb + n_frames, nullptr);
    const int threads = std::min(n_frames, mpc::host_thread_count());
    std::vector<std::thread> workers;
    workers.reserve(static_cast<size_t>(threads));
    for (int k = 1; k < threads; ++k) workers.emplace_back([&q] { parse_worker(q); });
    parse_worker(q);
    for (std::thread& t : workers) t.join();
    if (q.failed_frame == INT_MAX) return MPC_OK;
    if (rgb)
        for (int f = 0; f < n_frames; ++f) {
            std::free(rgb[f]);
            rgb[f] = nullptr;
        }
    if (out_indexes)
        for (int f = 0; f < n_frames; ++f) {
            std::free(out_indexes[f]);
            out_indexes[f] = nullptr;
            out_index_bytes[f] = 0;
        }
    if (containers)
        for (int f = 0; f < n_frames; ++f) {
            std::free(containers[f]);
            containers[f] = nullptr;
            container_bytes[f] = 0;
        }
    if (q.single) return fail(q.failed_status, "%s", q.failed_text.c_str());
    if (compose) return fail(q.failed_status, "part %d: %s", compose->part_of_frame[q.failed_frame], q.failed_text.c_str());
    return fail(q.failed_status, "frame %d: %s", q.failed_frame, q.failed_text.c_str());
}

}  // namespace

extern "C" {

// compressed::decodeImage: one frame through the sequence decoder in its host form.  The stream's own K and quantisation table are
// used (they need not match the context's); there is no host reconstruction.
mpc_status mpc_decode_image(const mpc_context* c, const uint8_t* bytes, size_t nbytes, uint8_t** rgb, int* width, int* height) {
    return guarded([&]() -> mpc_status {
        if (!c || !bytes || !rgb || !width || !height) return fail(MPC_ERR_ARGUMENT, "null argument");
        return decode_sequence(const_cast<mpc_context*>(c), &bytes, &nbytes, 1, rgb, nullptr, nullptr, width, height, true);
    });
}

mpc_status mpc_decode_images(mpc_context* c, const uint8_t* const* bytes, const size_t* nbytes, int n_frames, uint8_t** rgb, int* width,
                             int* height) {
    return guarded([&]() -> mpc_status {
        if (!rgb) return fail(MPC_ERR_ARGUMENT, "null argument");
        return decode_sequence(c, bytes, nbytes, n_frames, rgb, nullptr, nullptr, width, height);
    });
}

mpc_status mpc_decode_images_device(mpc_context* c, const uint8_t* const* bytes, const size_t* nbytes, int n_frames, uint8_t* const* d_rgb,
                                    const size_t* capacity, int* width, int* height) {
    return guarded([&]() -> mpc_status {
        if (!d_rgb) return fail(MPC_ERR_ARGUMENT, "null argument");
        return decode_sequence(c, bytes, nbytes, n_frames, nullptr, d_rgb, capacity, width, height);
    });
}

mpc_status mpc_decode_image_device(mpc_context* c, const uint8_t* bytes, size_t nbytes, uint8_t* d_rgb, size_t capacity, int* width,
                                   int* height) {
    return mpc_decode_images_device(c, &bytes, &nbytes, 1, &d_rgb, &capacity, width, height);
}

mpc_status mpc_decode_images_indexed(mpc_context* c, const uint8_t* const* bytes, const size_t* nbytes, const uint8_t* const* indexes,
                                     const size_t* index_bytes, int n_frames, uint8_t** rgb, int* width, int* height, int* routes) {
    return guarded([&]() -> mpc_status {
        if (!rgb) return fail(MPC_ERR_ARGUMENT, "null argument");
        return decode_sequence(c, bytes, nbytes, n_frames, rgb, nullptr, nullptr, width, height, false, indexes, index_bytes, routes);
    });
}

mpc_status mpc_decode_images_indexed_device(mpc_context* c, const uint8_t* const* bytes, const size_t* nbytes, const uint8_t* const* indexes,
                                            const size_t* index_bytes, int n_frames, uint8_t* const* d_rgb, const size_t* capacity,
                                            int* width, int* height, int* routes) {
    return guarded([&]() -> mpc_status {
        if (!d_rgb) return fail(MPC_ERR_ARGUMENT, "null argument");
        return decode_sequence(c, bytes, nbytes, n_frames, nullptr, d_rgb, capacity, width, height, false, indexes, index_bytes, routes);
    });
}

mpc_status mpc_decode_images_scan(mpc_context* c, const uint8_t* const* bytes, const size_t* nbytes, int n_frames, uint8_t** rgb, int* width,
                                  int* height, uint8_t** indexes, size_t* index_bytes, int* routes) {
    return guarded([&]() -> mpc_status {
        if (!rgb) return fail(MPC_ERR_ARGUMENT, "null argument");
        return decode_sequence(c, bytes, nbytes, n_frames, rgb, nullptr, nullptr, width, height, false, nullptr, nullptr, routes, nullptr, 0, nullptr,
                               true, indexes, index_bytes);
    });
}

mpc_status mpc_decode_images_scan_device(mpc_context* c, const uint8_t* const* bytes, const size_t* nbytes, int n_frames, uint8_t* const* d_rgb,
                                         const size_t* capacity, int* width, int* height, uint8_t** indexes, size_t* index_bytes, int* routes) {
    return guarded([&]() -> mpc_status {
        if (!d_rgb) return fail(MPC_ERR_ARGUMENT, "null argument");
        return decode_sequence(c, bytes, nbytes, n_frames, nullptr, d_rgb, capacity, width, height, false, nullptr, nullptr, routes, nullptr, 0,
                               nullptr, true, indexes, index_bytes);
    });
}

mpc_status mpc_decode_regions_indexed(mpc_context* c, const uint8_t* const* bytes, const size_t* nbytes, const uint8_t* const* indexes,
                                      const size_t* index_bytes, const mpc_rect* rects, int n_frames, unsigned flags, uint8_t** rgb,
                                      int* routes) {
    return guarded([&]() -> mpc_status {
        if (!rgb || !rects) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (flags & ~MPC_REGION_PARSE_ALL) return fail(MPC_ERR_ARGUMENT, "flags 0x%x", flags);
        std::vector<int> wh(2 * static_cast<size_t>(std::max(n_frames, 1)));
        return decode_sequence(c, bytes, nbytes, n_frames, rgb, nullptr, nullptr, wh.data(), wh.data() + std::max(n_frames, 1), false, indexes,
                               index_bytes, routes, rects, flags);
    });
}

mpc_status mpc_decode_regions_indexed_device(mpc_context* c, const uint8_t* const* bytes, const size_t* nbytes, const uint8_t* const* indexes,
                                             const size_t* index_bytes, const mpc_rect* rects, int n_frames, unsigned flags,
                                             uint8_t* const* d_rgb, const size_t* capacity, int* routes) {
    return guarded([&]() -> mpc_status {
        if (!d_rgb || !rects) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (flags & ~MPC_REGION_PARSE_ALL) return fail(MPC_ERR_ARGUMENT, "flags 0x%x", flags);
        std::vector<int> wh(2 * static_cast<size_t>(std::max(n_frames, 1)));
        return decode_sequence(c, bytes, nbytes, n_frames, nullptr, d_rgb, capacity, wh.data(), wh.data() + std::max(n_frames, 1), false,
                               indexes, index_bytes, routes, rects, flags);
    });
}

namespace {
// The views' arguments checked ("frame N: ...") and their rectangles resolved against the containers' headers, then the sequence.  A
// frame whose header does not parse gets a placeholder: it fails in its turn, as in every other call
mpc_status decode_views(mpc_context* c, const uint8_t* const* bytes, const size_t* nbytes, const uint8_t* const* indexes, const size_t* index_bytes,
                        const mpc_view* views, int n_frames, unsigned flags, uint8_t** rgb, uint8_t* const* d_rgb, const size_t* capacity,
                        int* width, int* height, int* routes) {
    if (!views || !bytes || !nbytes) return fail(MPC_ERR_ARGUMENT, "null argument");
    if (flags & ~MPC_VIEW_PARSE_ALL) return fail(MPC_ERR_ARGUMENT, "flags 0x%x", flags);
    if (n_frames < 1) return fail(MPC_ERR_ARGUMENT, "n_frames must be at least 1");
    std::vector<mpc_rect> rects(static_cast<size_t>(n_frames));
    for (int f = 0; f < n_frames; ++f) {
        if (!bytes[f]) return fail(MPC_ERR_ARGUMENT, "frame %d: null argument", f);
        if (const char* why = view_argument_error(views[f])) return fail(MPC_ERR_ARGUMENT, "frame %d: %s", f, why);
        int w, h, K, bs;
        rects[static_cast<size_t>(f)] = mpc::container_info(bytes[f], nbytes[f], &w, &h, &K, &bs) ? view_rect(views[f], w, h) : mpc_rect{0, 0, 1, 1};
    }
    static_assert(MPC_VIEW_PARSE_ALL == MPC_REGION_PARSE_ALL, "the sequence knows one parse-all flag");
    return decode_sequence(c, bytes, nbytes, n_frames, rgb, d_rgb, capacity, width, height, false, indexes, index_bytes, routes, rects.data(),
                           flags, views);
}
}  // namespace

mpc_status mpc_decode_views_indexed(mpc_context* c, const uint8_t* const* bytes, const size_t* nbytes, const uint8_t* const* indexes,
                                    const size_t* index_bytes, const mpc_view* views, int n_frames, unsigned flags, uint8_t** rgb, int* width,
                                    int* height, int* routes) {
    return guarded([&]() -> mpc_status {
        if (!rgb) return fail(MPC_ERR_ARGUMENT, "null argument");
        return decode_views(c, bytes, nbytes, indexes, index_bytes, views, n_frames, flags, rgb, nullptr, nullptr, width, height, routes);
    });
}

mpc_status mpc_decode_views_indexed_device(mpc_context* c, const uint8_t* const* bytes, const size_t* nbytes, const uint8_t* const* indexes,
                                           const size_t* index_bytes, const mpc_view* views, int n_frames, unsigned flags,
                                           uint8_t* const* d_rgb, const size_t* capacity, int* width, int* height, int* routes) {
    return guarded([&]() -> mpc_status {
        if (!d_rgb) return fail(MPC_ERR_ARGUMENT, "null argument");
        return decode_views(c, bytes, nbytes, indexes, index_bytes, views, n_frames, flags, nullptr, d_rgb, capacity, width, height, routes);
    });
}

// A transcode (include/mpcodec.h, "transcode"): the view decoder's sequence up to the gather, then the crop kernel and the
// records-to-container chain instead of the reconstruction (transcode_on_slot).  Arguments that need no device are checked first,
// "frame N: ...", with mpc_transcode_container's own texts
mpc_status mpc_transcode_views_indexed(mpc_context* c, const uint8_t* const* bytes, const size_t* nbytes, const uint8_t* const* indexes,
                                       const size_t* index_bytes, const mpc_view* views, int n_frames, unsigned flags, uint8_t** out,
                                       size_t* out_bytes, int* routes) {
    return guarded([&]() -> mpc_status {
        if (!c || !views || !bytes || !nbytes || !out || !out_bytes) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (flags & ~MPC_VIEW_PARSE_ALL) return fail(MPC_ERR_ARGUMENT, "flags 0x%x", flags);
        if (n_frames < 1) return fail(MPC_ERR_ARGUMENT, "n_frames must be at least 1");
        std::fill(out, out + n_frames, nullptr);
        std::fill(out_bytes, out_bytes + n_frames, 0);
        if (c->device < 0) return no_device();
        std::vector<mpc_rect> rects(static_cast<size_t>(n_frames));
        for (int f = 0; f < n_frames; ++f) {
            if (!bytes[f]) return fail(MPC_ERR_ARGUMENT, "frame %d: null argument", f);
            if (const char* why = transcode_argument_error(views[f])) return fail(MPC_ERR_ARGUMENT, "frame %d: %s", f, why);
            int w, h, K, bs;
            if (!mpc::container_info(bytes[f], nbytes[f], &w, &h, &K, &bs)) {           // fails in its turn, as in every other call
                rects[static_cast<size_t>(f)] = mpc_rect{0, 0, 1, 1};
                continue;
            }
            const mpc_rect r = view_rect(views[f], w, h);
            const std::string why = mpc::transcode_rect_error(w, h, bs, r.x, r.y, r.width, r.height);
            if (!why.empty()) return fail(MPC_ERR_ARGUMENT, "frame %d: %s", f, why.c_str());
            rects[static_cast<size_t>(f)] = r;
        }
        std::vector<int> wh(2 * static_cast<size_t>(n_frames));
        return decode_sequence(c, bytes, nbytes, n_frames, nullptr, nullptr, nullptr, wh.data(), wh.data() + n_frames, false, indexes, index_bytes,
                               routes, rects.data(), flags, views, false, nullptr, nullptr, out, out_bytes);
    });
}

// A compose (include/mpcodec.h, "compose"): the host's plan (every check that needs no device, the owner map), then per owning part
// either the view decoder's sequence up to the gather with the paste kernel behind it (paste_on_slot) or, for pixels, the tile encode
// into a patch of records and the same kernel; one records-to-container job on job slot 0 once every paste has finished
mpc_status mpc_compose_indexed(mpc_context* c, const uint8_t* const* bytes, const size_t* nbytes, const uint8_t* const* indexes,
                               const size_t* index_bytes, int n_sources, const mpc_part* parts, int n_parts, int width, int height,
                               unsigned flags, int index_interval, uint8_t** out, size_t* out_bytes, uint8_t** index, size_t* index_out_bytes,
                               int* routes) {
    return guarded([&]() -> mpc_status {
        if (!c || !parts || !out || !out_bytes || !routes || (n_sources > 0 && (!bytes || !nbytes)) || (indexes && !index_bytes))
            return fail(MPC_ERR_ARGUMENT, "null argument");
        if (index_interval >= 0 && (!index || !index_out_bytes)) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (flags & ~(MPC_VIEW_PARSE_ALL | MPC_COMPOSE_DEVICE_PIXELS)) return fail(MPC_ERR_ARGUMENT, "flags 0x%x", flags);
        unsigned every = 0;
        if (const mpc_status bad = optional_index_interval_of(index_interval, &every)) return bad;
        *out = nullptr;
        *out_bytes = 0;
        if (index) *index = nullptr;
        if (index_out_bytes) *index_out_bytes = 0;
        if (c->device < 0) return no_device();
        const std::vector<mpc::ComposePart> pieces = compose_parts(parts, n_parts);
        const mpc::ComposeDevice device{c->K, c->block_size};
        mpc::ComposePlan plan;
        std::string why;
        if (const int verdict = mpc::compose_plan(bytes, nbytes, n_sources, pieces.data(), n_parts, width, height, &device, plan, why); verdict != 0)
            return fail(verdict == 1 ? MPC_ERR_BITSTREAM : MPC_ERR_ARGUMENT, "%s", why.c_str());
        const int K = c->K, bs = c->block_size;
        for (int p = 0; p < n_parts; ++p)
            if (parts[p].source == -1 && parts[p].row_stride != 0 && parts[p].row_stride < 3 * static_cast<size_t>(parts[p].rect.width))
                return fail(MPC_ERR_ARGUMENT, "part %d: row_stride %zu for %d pixels", p, parts[p].row_stride, parts[p].rect.width);
        struct Routes {                                             // on failure nothing is returned: no part has a route
            int* at;
            int n;
            bool keep = false;
            ~Routes() {
                if (!keep) std::fill(at, at + n, -1);
            }
        } told{routes, n_parts};
        std::fill(routes, routes + n_parts, -1);
        // the destination's quantiser table: source 0's header values, which the tile encode of a pixel part quantises with as well
        std::vector<double> table;
        if (n_sources > 0)
            for (int ch = 0; ch < 3; ++ch)
                for (int i = 0; i < K; ++i) table.push_back(static_cast<double>(plan.sources[0].quant[ch][i]));
        const double* quant = n_sources > 0 ? table.data() : nullptr;                // null: the context's, as its encoder writes them
        std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
        HIP_TRY(hipSetDevice(c->device));
        const Tuning tuning = read_tuning();
        for (int k = 0; k < mpc_context::kSeqSlots; ++k)
            if (c->jobs[k] && c->jobs[k]->stage != 0) return fail(MPC_ERR_ARGUMENT, "container job slot %d is busy", k);
        if (!c->jobs[0]) c->jobs[0] = std::make_unique<JobSlot>();
        JobSlot& js = *c->jobs[0];
        ContainerJob& job = js.job;
        if (!job.phase1) {
            HIP_TRY(hipEventCreateWithFlags(&job.phase1, hipEventDisableTiming | hipEventBlockingSync));
            HIP_TRY(hipEventCreateWithFlags(&job.done, hipEventDisableTiming | hipEventBlockingSync));
        }
        // the destination's records and the owner map: every word of the records is written exactly once, by its tile's owner.  They,
        // the pixel parts' pixels and their patches of records live in one grow-only buffer of the context: free in steady state
        const size_t tiles = plan.owner.size(), n_tc = 3 * tiles;
        const bool upload = !(flags & MPC_COMPOSE_DEVICE_PIXELS);
        struct Patch {
            uint8_t* d_rgb = nullptr;
            uint16_t* d_counts = nullptr;
            mpc_basis_choice* d_choices = nullptr;
        };
        std::vector<Patch> patches(static_cast<size_t>(n_parts));
        ComposeTarget to;
        int32_t* d_owner = nullptr;
        const auto layout = [&](char* base) {
            Carve cv{base};
            to.d_counts = cv.take<uint16_t>(n_tc + 2);
            to.d_choices = cv.take<uint32_t>(n_tc * static_cast<size_t>(K));
            d_owner = cv.take<int32_t>(tiles + 1);                  // behind the map the pixel parts' error word
            for (int p = 0; p < n_parts; ++p) {
                const mpc::ComposePart& piece = plan.parts[static_cast<size_t>(p)];
                if (piece.source != -1 || !plan.owns[static_cast<size_t>(p)]) continue;
                Patch& patch = patches[static_cast<size_t>(p)];
                const size_t patch_tc = 3 * static_cast<size_t>((piece.w + bs - 1) / bs) * static_cast<size_t>((piece.h + bs - 1) / bs);
                if (upload) patch.d_rgb = cv.take<uint8_t>(3 * static_cast<size_t>(piece.w) * static_cast<size_t>(piece.h));
                patch.d_counts = cv.take<uint16_t>(patch_tc + 2);
                patch.d_choices = cv.take<mpc_basis_choice>(patch_tc * static_cast<size_t>(K));
            }
            return cv.at;
        };
        if (const mpc_status gs = c->compose_dev.reserve(layout(nullptr), "compose staging"); gs != MPC_OK) return gs;
        layout(c->compose_dev.data());
        if (!c->compose_side) HIP_TRY(hipStreamCreateWithFlags(&c->compose_side, hipStreamNonBlocking));
        struct Side {                                               // the pixel parts' stream, later the job's: drained whatever happens
            hipStream_t s;
            ~Side() { (void)hipStreamSynchronize(s); }
        } side{c->compose_side};
        plan.owner.push_back(0);                                    // the error word, cleared
        HIP_TRY(hipMemcpy(d_owner, plan.owner.data(), sizeof(int32_t) * (tiles + 1), hipMemcpyHostToDevice));
        int* d_error = d_owner + tiles;                             // no encoder writes a count above K
        to.d_owner = d_owner;
        to.tiles_x = plan.tiles_x;
        to.tiles_y = plan.tiles_y;
        to.parts = plan.parts.data();
        // pixel parts: a frame of their own through the tile encode, on the side stream beside the container parts
        for (int p = 0; p < n_parts; ++p) {
            const mpc::ComposePart& piece = plan.parts[static_cast<size_t>(p)];
            if (piece.source != -1 || !plan.owns[static_cast<size_t>(p)]) continue;
            const Patch& patch = patches[static_cast<size_t>(p)];
            const size_t row = 3 * static_cast<size_t>(piece.w), stride = parts[p].row_stride ? parts[p].row_stride : row;
            if (upload) HIP_TRY(hipMemcpy2DAsync(patch.d_rgb, row, parts[p].rgb, stride, row, static_cast<size_t>(piece.h), hipMemcpyHostToDevice, side.s));
            const int ptx = (piece.w + bs - 1) / bs, pty = (piece.h + bs - 1) / bs;
            if (const mpc_status es = mpc_encode_tiles_device(c, upload ? patch.d_rgb : parts[p].rgb, piece.w, piece.h, upload ? row : stride, 0, pty,
                                                              quant, patch.d_counts, patch.d_choices, nullptr, nullptr, 0, side.s);
                es != MPC_OK)
                return es;
            if (const int e = mpc::launch_paste_records(patch.d_counts, reinterpret_cast<const uint32_t*>(patch.d_choices), ptx, pty, 0, 0, ptx, pty, K,
                                                        to.d_counts, to.d_choices, to.tiles_x, to.tiles_y, piece.dx / bs, piece.dy / bs, to.d_owner, p,
                                                        d_error, side.s);
                e != 0)
                return launch_failed(e);
            routes[p] = 2;
        }
        // container parts that own a tile: the frames of one sequence on the decode slots, in part order
        std::vector<int> part_of_frame;
        for (int p = 0; p < n_parts; ++p)
            if (plan.parts[static_cast<size_t>(p)].source >= 0 && plan.owns[static_cast<size_t>(p)]) part_of_frame.push_back(p);
        const int n_frames = static_cast<int>(part_of_frame.size());
        mpc_status st = MPC_OK;
        if (n_frames > 0) {
            const size_t n = static_cast<size_t>(n_frames);
            std::vector<const uint8_t*> f_bytes(n), f_index(n, nullptr);
            std::vector<size_t> f_nbytes(n), f_index_bytes(n, 0);
            std::vector<mpc_rect> f_rects(n);
            std::vector<mpc_view> f_views(n);
            std::vector<int> f_routes(n, 1), wh(2 * n);
            for (size_t f = 0; f < n; ++f) {
                const mpc::ComposePart& piece = plan.parts[static_cast<size_t>(part_of_frame[f])];
                f_bytes[f] = bytes[piece.source];
                f_nbytes[f] = nbytes[piece.source];
                if (indexes && indexes[piece.source]) {
                    f_index[f] = indexes[piece.source];
                    f_index_bytes[f] = index_bytes[piece.source];
                }
                f_rects[f] = mpc_rect{piece.x, piece.y, piece.w, piece.h};
                f_views[f] = mpc_view{f_rects[f], 0, 0};
            }
            to.part_of_frame = part_of_frame.data();
            st = decode_sequence(c, f_bytes.data(), f_nbytes.data(), n_frames, nullptr, nullptr, nullptr, wh.data(), wh.data() + n, false,
                                 f_index.data(), f_index_bytes.data(), f_routes.data(), f_rects.data(), flags & MPC_VIEW_PARSE_ALL, f_views.data(),
                                 false, nullptr, nullptr, nullptr, nullptr, &to);
            if (st == MPC_OK)
                for (size_t f = 0; f < n; ++f) routes[part_of_frame[f]] = f_routes[f];
        }
        if (st == MPC_OK) {
            int flag = 0;
            HIP_TRY(hipMemcpyAsync(&flag, d_error, sizeof(int), hipMemcpyDeviceToHost, side.s));
            HIP_TRY(hipStreamSynchronize(side.s));                  // every paste has finished: the container parts' on their slots' events
            if (flag) st = fail(MPC_ERR_BITSTREAM, "Invalid bitstream");
        }
        if (st != MPC_OK) return st;
        // records -> container on job slot 0, with the seek index from the entropy stage where one is asked for
        Carve measure;
        mpc::StreamArgs measured{};
        carve_stream_buffers(measure, static_cast<long long>(tiles), K, true, &measured);
        if (const mpc_status gs = js.dev.reserve(measure.at, "device staging"); gs != MPC_OK) return gs;
        GrowBuffer host_stage(GrowBuffer::kPinned);                 // the host route's, should the frame take it: this call's own
        job.side = job.down = side.s;
        job.spin = true;
        job.host_stage = &host_stage;
        job.host_offset = 0;
        job.index_interval = every;
        job.index_expanded = every != 0;
        struct Unhook {                                             // the slot is left as mpc_container_job_begin expects it
            ContainerJob& job;
            ~Unhook() {
                job.host_stage = nullptr;
                job.index_interval = 0;
                job.index_expanded = false;
                job.index.clear();
            }
        } unhook{job};
        EntropyBuffers eb;
        if (!tuning.host_entropy)
            if (const mpc_status es = entropy_buffers(js.ent, tiles, K, &eb, every ? 2 : 0); es != MPC_OK) return es;
        HIP_TRY(hipStreamSynchronize(nullptr));                     // a slot carved for another geometry clears its tables on the null stream
        if (const mpc_status bs_ = container_begin(job, c, tuning.host_entropy ? nullptr : &eb, tuning.triple_limit, js.dev.data(), to.d_counts,
                                                   to.d_choices, nullptr, nullptr, width, height, quant);
            bs_ != MPC_OK)
            return bs_;
        if (const mpc_status ts = container_tables(job); ts != MPC_OK) return ts;
        uint8_t* made = nullptr;
        size_t made_bytes = 0;
        if (const mpc_status cs = container_collect(job, &made, &made_bytes); cs != MPC_OK) return cs;
        if (hipStreamSynchronize(side.s) != hipSuccess) {
            std::free(made);
            return fail(MPC_ERR_HIP, "the container job failed: %s", hipGetErrorString(hipGetLastError()));
        }
        if (every) {
            uint8_t* copy = job.index.empty() ? nullptr : static_cast<uint8_t*>(std::malloc(job.index.size()));
            if (!copy) {
                std::free(made);
                return fail(MPC_ERR_ALLOC, "no seek index");
            }
            std::memcpy(copy, job.index.data(), job.index.size());
            *index = copy;
            *index_out_bytes = job.index.size();
        }
        *out = made;
        *out_bytes = made_bytes;
        told.keep = true;
        return MPC_OK;
    });
}

}  // extern "C"

namespace {
// mpc_parse_container_window_device (symbols, n_symbols, ranges) and mpc_window_chunks_device (chunks): one run of the device half
mpc_status window_on_device(mpc_context* c, const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes,
                            const mpc_rect* rect, unsigned flags, uint16_t** symbols, size_t* n_symbols, uint64_t* ranges, uint64_t* chunks,
                            int* route, int steps = 0) {
    // steps (mpc_parse_container_view_device, never with `chunks`): a view's, 0 = every step
    return guarded([&]() -> mpc_status {
        if (!c || !bytes || !index || !rect || !route || (chunks ? false : !symbols || !n_symbols || !ranges)) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (flags & ~MPC_REGION_PARSE_ALL) return fail(MPC_ERR_ARGUMENT, "flags 0x%x", flags);
        if (c->device < 0) return no_device();
        const bool parse_all = (flags & MPC_REGION_PARSE_ALL) != 0;
        const auto give = [&](const std::vector<uint16_t>& got) -> mpc_status {
            uint16_t* out = static_cast<uint16_t*>(std::malloc(got.empty() ? 2 : 2 * got.size()));
            if (!out) return fail(MPC_ERR_ALLOC, "out of memory");
            if (!got.empty()) std::memcpy(out, got.data(), 2 * got.size());
            *symbols = out;
            *n_symbols = got.size();
            return MPC_OK;
        };
        // every refusal of the index: the host definition's own route 1 (no index at all)
        const auto serial = [&]() -> mpc_status {
            if (chunks) {
                std::vector<uint64_t> none;
                const int verdict = mpc::window_chunks_by_index(bytes, nbytes, nullptr, 0, rect->x, rect->y, rect->width, rect->height, parse_all, none, route);
                if (verdict == 1) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
                if (verdict == 2)
                    return fail(MPC_ERR_ARGUMENT, "rectangle %dx%d at (%d, %d) is empty or not inside the frame", rect->width, rect->height, rect->x, rect->y);
                std::memcpy(chunks, none.data(), sizeof(uint64_t) * none.size());
                return MPC_OK;
            }
            std::vector<uint16_t> got;
            std::vector<uint64_t> r;
            const int verdict = mpc::read_window_by_index(bytes, nbytes, nullptr, 0, rect->x, rect->y, rect->width, rect->height, parse_all, got, r, route, steps);
            if (verdict == 1) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
            if (verdict == 2)
                return fail(MPC_ERR_ARGUMENT, "rectangle %dx%d at (%d, %d) is empty or not inside the frame", rect->width, rect->height, rect->x, rect->y);
            std::memcpy(ranges, r.data(), sizeof(uint64_t) * r.size());
            return give(got);
        };
        ParsePlan pp;
        if (!plan_parse(bytes, nbytes, index, index_bytes, false, pp, parse_all ? 0 : steps)) return serial();
        const mpc::ContainerIndex& x = pp.ip.index;
        const int kept = view_steps(steps, x.K);                    // the lengths are cut to it on the device, unless "parse all"
        mpc::TileWindow win;
        if (!mpc::tile_window(x.width, x.height, x.block_size, rect->x, rect->y, rect->width, rect->height, win)) return serial();
        std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
        HIP_TRY(hipSetDevice(c->device));
        if (const mpc_status ss = ensure_slots(c, 1); ss != MPC_OK) return ss;
        DecodeSlot& slot = *c->dec[0];
        const int K = x.K;
        const size_t n_counts = pp.n_counts, n_out = pp.unpack.n_symbols, n_streams = 6 * static_cast<size_t>(K);
        mpc::StreamArgs sa{};
        mpc::WindowStream* d_window;
        mpc::WindowSpan* d_span = nullptr;
        const bool cut = pp.expanded && !parse_all;
        auto behind_layout = [&](char* base) {
            Carve cv{base};
            carve_stream_buffers(cv, static_cast<long long>(pp.ip.tiles), K, false, &sa);
            d_window = cv.take<mpc::WindowStream>(n_streams);
            if (cut) d_span = cv.take<mpc::WindowSpan>(n_streams);
            return cv.at;
        };
        uint16_t* h_counts;
        uint16_t* h_symbols;
        mpc::WindowStream* h_window;
        auto result_layout = [&](char* base) {
            Carve cv{base};
            h_counts = cv.take<uint16_t>(n_counts + 2);
            h_symbols = cv.take<uint16_t>(n_out + 2);
            h_window = cv.take<mpc::WindowStream>(n_streams);
            return cv.at;
        };
        UnpackJob j;
        j.plan = &pp.unpack;
        j.K = K;
        j.behind_bytes = behind_layout(nullptr);
        j.result_bytes = result_layout(nullptr);
        mpc::ParseArgs pa{};
        if (const mpc_status us = upload_and_parse(slot, j, pp, bytes, nbytes, &pa, cut); us != MPC_OK) return us;
        behind_layout(j.d_behind);
        result_layout(j.h_result);
        if (const mpc_status ws = parse_and_unpack_window(slot, j, pp, pa, sa, d_window, win, parse_all, d_span, chunks != nullptr,
                                                          !parse_all && kept < K ? kept : 0);
            ws != MPC_OK)
            return ws;
        hipStream_t st = slot.stream;
        HIP_TRY(hipMemcpyAsync(j.h_flags, j.ua.error, 3 * sizeof(int), hipMemcpyDeviceToHost, st));
        if (!chunks) {
            HIP_TRY(hipMemcpyAsync(h_counts, pa.counts, sizeof(uint16_t) * n_counts, hipMemcpyDeviceToHost, st));
            if (n_out) HIP_TRY(hipMemcpyAsync(h_symbols, j.ua.symbols, sizeof(uint16_t) * n_out, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipMemcpyAsync(h_window, d_window, sizeof(mpc::WindowStream) * n_streams, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(slot.done, st));
        HIP_TRY(hipEventSynchronize(slot.done));
        if (chunks) {                                               // the rank kernel's table; nothing behind that kernel was launched
            if (j.h_flags[2] != 0) return serial();                 // the lengths are not what the index says: the host's route 1
            for (size_t i = 0; i < n_streams; ++i) {
                chunks[2 * i] = h_window[i].c0;
                chunks[2 * i + 1] = h_window[i].c1;
            }
            *route = 0;
            return MPC_OK;
        }
        if (j.h_flags[2] != 0 || j.h_flags[0] != 0) return serial();
        // the window's slice of every expanded stream; (r0, r1) are the device's, held to the host's sizes
        std::vector<uint16_t> got(h_counts, h_counts + n_counts);
        for (uint16_t& length : got) length = std::min<uint16_t>(length, static_cast<uint16_t>(kept));     // "parse all": not cut on the device
        for (size_t i = 0; i < n_streams; ++i) {
            const mpc::UnpackStream& us = pp.unpack.table[i];
            const bool cut_away = static_cast<int>((i % (2 * static_cast<size_t>(K))) / 2) >= kept;          // ... nor are its ranks
            const unsigned long long r1 = cut_away ? 0 : std::min<unsigned long long>(h_window[i].r1, us.expect),
                                     r0 = std::min<unsigned long long>(h_window[i].r0, r1);
            got.insert(got.end(), h_symbols + us.out_off + r0, h_symbols + us.out_off + r1);
            ranges[2 * (i / 2)] = r0;
            ranges[2 * (i / 2) + 1] = r1;
        }
        *route = 0;
        return give(got);
    });
}
}  // namespace

// mpc_container_index_device and its debug form: the device scan proposes, the device parse (the decoder's own upload-and-parse
// step, on the bytes the scan has put on the slot) decides; whatever either refuses, the serial builder answers
mpc_status container_index_on_device(mpc_context* c, const uint8_t* bytes, size_t nbytes, int interval, unsigned flags, int segment_bits,
                                     int window_bits, uint8_t** index, size_t* index_bytes, int* route) {
    return guarded([&]() -> mpc_status {
        if (!c || !bytes || !index || !index_bytes || !route) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (flags & ~MPC_INDEX_EXPANDED) return fail(MPC_ERR_ARGUMENT, "flags 0x%x", flags);
        if (interval != 0 && (interval < static_cast<int>(mpc::kIndexIntervalMin) || interval > static_cast<int>(mpc::kIndexIntervalMax)))
            return fail(MPC_ERR_ARGUMENT, "interval %d: 0 or %u to %u", interval, mpc::kIndexIntervalMin, mpc::kIndexIntervalMax);
        uint32_t segment = segment_bits < 0 ? 1u : static_cast<uint32_t>(segment_bits), window = window_bits < 0 ? 1u : static_cast<uint32_t>(window_bits);
        if (!mpc::scan_sizes_ok(&segment, &window))
            return fail(MPC_ERR_ARGUMENT, "segment of %d bits, window of %d: 0, or a segment of %u to %u bits and a window of whole segments up to %u bits",
                        segment_bits, window_bits, mpc::kScanSegmentMin, mpc::kScanSegmentMax, mpc::kScanWindowMax);
        if (c->device < 0) return no_device();
        const bool expanded = (flags & MPC_INDEX_EXPANDED) != 0;
        std::vector<uint8_t> blob;
        const auto give = [&]() -> mpc_status {
            uint8_t* p = static_cast<uint8_t*>(std::malloc(blob.empty() ? 1 : blob.size()));
            if (!p) return fail(MPC_ERR_ALLOC, "out of memory");
            if (!blob.empty()) std::memcpy(p, blob.data(), blob.size());
            *index = p;
            *index_bytes = blob.size();
            return MPC_OK;
        };
        const auto serial = [&]() -> mpc_status {
            *route = 1;
            blob.clear();
            if (!mpc::build_container_index(bytes, nbytes, static_cast<uint32_t>(interval), blob, expanded)) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
            return give();
        };
        std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
        HIP_TRY(hipSetDevice(c->device));
        if (const mpc_status ss = ensure_slots(c, 1); ss != MPC_OK) return ss;
        DecodeSlot& slot = *c->dec[0];
        const bool trace = read_tuning().trace;
        bool proposed = false;
        if (const mpc_status ps = scan_on_slot(slot, bytes, nbytes, static_cast<uint32_t>(interval), segment, window, true, trace, blob, &proposed); ps != MPC_OK)
            return ps;
        if (!proposed) return serial();
        ParsePlan pp;
        if (!plan_parse(bytes, nbytes, blob.data(), blob.size(), true, pp)) return serial();
        UnpackJob j;
        j.plan = &pp.unpack;
        j.K = pp.ip.index.K;
        j.pooled = true;
        if (const mpc_status us = upload_and_parse(slot, j, pp, bytes, nbytes, nullptr, false, true); us != MPC_OK) return us;
        hipStream_t st = slot.stream;
        HIP_TRY(hipMemcpyAsync(j.h_flags, j.ua.error, 3 * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(slot.done, st));
        HIP_TRY(hipEventSynchronize(slot.done));
        if (j.h_flags[2] != 0) return serial();
        // accepted: the serial parser's path, so the serial builder's version-1 blob
        if (!mpc::accept_proposed_index(bytes, nbytes, blob, expanded)) return serial();
        *route = 0;
        return give();
    });
}

extern "C" {

mpc_status mpc_parse_container_window_device(mpc_context* c, const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes,
                                             const mpc_rect* rect, unsigned flags, uint16_t** symbols, size_t* n_symbols, uint64_t* ranges,
                                             int* route) {
    if (!symbols || !n_symbols || !ranges) return guarded([&]() -> mpc_status { return fail(MPC_ERR_ARGUMENT, "null argument"); });
    return window_on_device(c, bytes, nbytes, index, index_bytes, rect, flags, symbols, n_symbols, ranges, nullptr, route);
}

mpc_status mpc_parse_container_view_device(mpc_context* c, const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes,
                                           const mpc_view* view, unsigned flags, uint16_t** symbols, size_t* n_symbols, uint64_t* ranges,
                                           int* route) {
    mpc_rect rect{};
    const mpc_status args = guarded([&]() -> mpc_status {
        if (!bytes || !view || !symbols || !n_symbols || !ranges) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (const char* why = view_argument_error(*view)) return fail(MPC_ERR_ARGUMENT, "%s", why);
        int w, h, K, bs;
        if (!mpc::container_info(bytes, nbytes, &w, &h, &K, &bs)) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
        rect = view_rect(*view, w, h);
        return MPC_OK;
    });
    if (args != MPC_OK) return args;
    static_assert(MPC_VIEW_PARSE_ALL == MPC_REGION_PARSE_ALL, "window_on_device knows one parse-all flag");
    return window_on_device(c, bytes, nbytes, index, index_bytes, &rect, flags, symbols, n_symbols, ranges, nullptr, route, view->steps);
}

mpc_status mpc_window_chunks_device(mpc_context* c, const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes,
                                    const mpc_rect* rect, unsigned flags, uint64_t* chunks, int* route) {
    if (!chunks) return guarded([&]() -> mpc_status { return fail(MPC_ERR_ARGUMENT, "null argument"); });
    return window_on_device(c, bytes, nbytes, index, index_bytes, rect, flags, nullptr, nullptr, nullptr, chunks, route);
}

mpc_status mpc_parse_container_device(mpc_context* c, const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes,
                                      uint16_t** symbols, size_t* n_symbols, int* route) {
    return guarded([&]() -> mpc_status {
        if (!c || !bytes || !index || !symbols || !n_symbols || !route) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (c->device < 0) return no_device();
        // the serial parse's result in this call's form: what every refusal of the index comes down to
        const auto serial = [&]() -> mpc_status {
            *route = 1;
            mpc::CodedStreams s;
            if (!mpc::read_compressed_coded(bytes, nbytes, s)) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
            size_t total = s.lengths.size();
            for (const std::vector<uint16_t>& v : s.codes) total += v.size();
            uint16_t* out = static_cast<uint16_t*>(std::malloc(total ? 2 * total : 2));
            if (!out) return fail(MPC_ERR_ALLOC, "out of memory");
            size_t at = 0;
            if (!s.lengths.empty()) std::memcpy(out, s.lengths.data(), 2 * s.lengths.size());
            at += s.lengths.size();
            for (const std::vector<uint16_t>& v : s.codes) {
                if (!v.empty()) std::memcpy(out + at, v.data(), 2 * v.size());
                at += v.size();
            }
            *symbols = out;
            *n_symbols = total;
            return MPC_OK;
        };
        ParsePlan pp;
        if (!plan_parse(bytes, nbytes, index, index_bytes, false, pp)) return serial();
        std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
        HIP_TRY(hipSetDevice(c->device));
        if (const mpc_status ss = ensure_slots(c, 1); ss != MPC_OK) return ss;
        DecodeSlot& slot = *c->dec[0];
        const size_t n_counts = pp.n_counts, n_coded = pp.unpack.n_coded;
        UnpackJob j;
        j.plan = &pp.unpack;
        j.K = pp.ip.index.K;
        j.result_bytes = sizeof(uint16_t) * (n_counts + n_coded + 2);
        if (const mpc_status us = upload_and_parse(slot, j, pp, bytes, nbytes); us != MPC_OK) return us;
        hipStream_t st = slot.stream;
        uint16_t* h_counts = reinterpret_cast<uint16_t*>(j.h_result);
        HIP_TRY(hipMemcpyAsync(j.h_flags, j.ua.error, 3 * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_counts, j.d_extra[0], sizeof(uint16_t) * n_counts, hipMemcpyDeviceToHost, st));
        if (n_coded) HIP_TRY(hipMemcpyAsync(h_counts + n_counts, j.ua.coded, sizeof(uint16_t) * n_coded, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(slot.done, st));
        HIP_TRY(hipEventSynchronize(slot.done));
        if (j.h_flags[2] != 0) return serial();
        const size_t total = n_counts + n_coded;
        uint16_t* out = static_cast<uint16_t*>(std::malloc(2 * total));
        if (!out) return fail(MPC_ERR_ALLOC, "out of memory");
        std::memcpy(out, h_counts, 2 * total);
        *symbols = out;
        *n_symbols = total;
        *route = 0;
        return MPC_OK;
    });
}

mpc_status mpc_container_index_device(mpc_context* c, const uint8_t* bytes, size_t nbytes, int interval, unsigned flags, uint8_t** index,
                                      size_t* index_bytes, int* route) {
    return container_index_on_device(c, bytes, nbytes, interval, flags, 0, 0, index, index_bytes, route);
}

mpc_status mpc_unpack_symbol_streams_device(mpc_context* c, int K, const uint16_t* coded, const unsigned long long* coded_off,
                                            const uint8_t* is_packed, const unsigned long long* expect, uint16_t** symbols,
                                            size_t* n_symbols) {
    return guarded([&]() -> mpc_status {
        if (!c || !coded_off || !is_packed || !expect || !symbols || !n_symbols) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (K < 1 || K > MPC_MAX_K) return fail(MPC_ERR_ARGUMENT, "K = %d", K);
        if (c->device < 0) return no_device();
        for (int i = 0; i < 6 * K; ++i)
            if (coded_off[i + 1] < coded_off[i]) return fail(MPC_ERR_ARGUMENT, "stream offsets must not decrease");
        if (coded_off[0] != 0 || (!coded && coded_off[6 * K])) return fail(MPC_ERR_ARGUMENT, "bad argument");
        UnpackPlan plan;
        if (!plan_unpack(K, [&](int i) { return coded_off[i + 1] - coded_off[i]; }, is_packed, expect, nullptr, plan))
            return fail(MPC_ERR_ARGUMENT, "streams too long");
        std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
        HIP_TRY(hipSetDevice(c->device));
        if (const mpc_status ss = ensure_slots(c, 1); ss != MPC_OK) return ss;
        DecodeSlot& slot = *c->dec[0];
        const size_t out_bytes = sizeof(uint16_t) * plan.n_symbols;
        UnpackJob j;
        j.plan = &plan;
        j.K = K;
        for (int i = 0; i < 6 * K; ++i) j.streams[i] = coded + coded_off[i];
        j.result_bytes = out_bytes;
        if (const mpc_status us = upload_and_unpack(slot, j); us != MPC_OK) return us;
        hipStream_t st = slot.stream;
        HIP_TRY(hipMemcpyAsync(j.h_flags, j.ua.error, sizeof(int), hipMemcpyDeviceToHost, st));
        if (out_bytes) HIP_TRY(hipMemcpyAsync(j.h_result, j.ua.symbols, out_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(slot.done, st));
        HIP_TRY(hipEventSynchronize(slot.done));
        if (j.h_flags[0] != 0) return fail(MPC_ERR_BITSTREAM, "Invalid bitstream");
        uint16_t* out = static_cast<uint16_t*>(std::malloc(out_bytes ? out_bytes : 2));
        if (!out) return fail(MPC_ERR_ALLOC, "out of memory");
        if (out_bytes) std::memcpy(out, j.h_result, out_bytes);
        *symbols = out;
        *n_symbols = plan.n_symbols;
        return MPC_OK;
    });
}

}  // extern "C"
