// mpcodec_decode_seq.cpp -- product: the C ABI's sequence decoder.  mpc_decode_image parses a container on one host thread
// while the device waits; nothing in the format is serial BETWEEN frames, so here the containers of a call are parsed side by
// side on threads of the call's own, each doing only what the format chains from code to code (mpc::read_compressed_coded: the
// entropy codes).  The coded streams cross PCIe and the per-symbol rest -- run-length expansion, DC sums -- happens on the
// device (mp_unpack.hip) in front of the gather and the reconstruction, frames pipelined over slots of their own streams.
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
    a->error = cv.take<int>(2);                                     // [1]: the reconstruction's error word
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
struct Sequence {
    mpc_context* c = nullptr;
    Tuning tuning;
    int n = 0, slots = 0;
    const uint8_t* const* bytes = nullptr;
    const size_t* nbytes = nullptr;
    uint8_t** rgb = nullptr;                    // host form: the results
    uint8_t* const* d_rgb = nullptr;            // device form: the caller's buffers
    const size_t* capacity = nullptr;
    int* width = nullptr;
    int* height = nullptr;
    std::atomic<int> next{0};                   // frames are handed out in order
    std::mutex lock;
    std::condition_variable turn;
    long long slot_uses[mpc_context::kDecodeSlots] = {};   // frame f owns slot f % slots once it has been used f / slots times
    int failed_frame = INT_MAX;                 // the first failing frame, its status and text
    mpc_status failed_status = MPC_OK;
    std::string failed_text;

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

// upload | unpack | gather | reconstruct | (host form) pixels down, on the slot's stream; returns with the frame complete
mpc_status frame_on_slot(Sequence& q, int f, DecodeSlot& slot, const mpc::CodedStreams& s, const UnpackPlan& plan, double stamps[3]) {
    mpc_context* c = q.c;
    const bool trace = q.tuning.trace;
    const int K = s.K;
    const size_t n_tc = s.lengths.size(), tiles = n_tc / 3;
    const size_t px = static_cast<size_t>(s.width) * s.height * 3;
    constexpr size_t kHead = 256;                                   // the pinned buffer's head: the two error words coming back
    uint16_t* counts;
    uint16_t* coded;
    mpc::UnpackStream* table;
    double* quant;
    auto upload_layout = [&](char* base) {
        Carve cv{base};
        counts = cv.take<uint16_t>(n_tc);
        coded = cv.take<uint16_t>(plan.n_coded + 2);
        table = cv.take<mpc::UnpackStream>(plan.table.size());
        quant = cv.take<double>(3 * static_cast<size_t>(K));
        return cv.at;
    };
    const size_t upload_bytes = upload_layout(nullptr);
    mpc::UnpackArgs ua{};
    mpc::StreamArgs sa{};
    uint32_t* d_choices;
    uint8_t* d_pixels = nullptr;
    auto device_layout = [&](char* base) {
        Carve cv{base};
        cv.at = upload_bytes;
        carve_unpack(cv, plan, K, &ua);
        d_choices = cv.take<uint32_t>(n_tc * K);
        carve_stream_buffers(cv, static_cast<long long>(tiles), K, false, &sa);
        if (!q.d_rgb) d_pixels = cv.take<uint8_t>(px);
        return cv.at;
    };
    if (const mpc_status gs = slot.pinned.reserve(kHead + std::max(upload_bytes, Carve::up(px)), "pinned decode staging"); gs != MPC_OK) return gs;
    if (const mpc_status gs = slot.dev.reserve(device_layout(nullptr), "device decode staging"); gs != MPC_OK) return gs;
    char* hbase = slot.pinned.data() + kHead;
    int* h_flags = reinterpret_cast<int*>(slot.pinned.data());
    upload_layout(hbase);
    // A call of one frame has no other frame's thread to share the cores with: its copies go through the worker pool, as
    // mpc_decode_image's do.  Otherwise every frame's thread copies its own.
    const bool pooled = q.n == 1;
    const auto stage = [&](int job) {
        if (job == 0) std::memcpy(counts, s.lengths.data(), sizeof(uint16_t) * n_tc);
        else if (!s.codes[job - 1].empty())
            std::memcpy(coded + plan.table[job - 1].coded_off, s.codes[job - 1].data(), sizeof(uint16_t) * s.codes[job - 1].size());
    };
    if (pooled) mpc::parallel_jobs(6 * K + 1, stage);
    else
        for (int job = 0; job <= 6 * K; ++job) stage(job);
    std::memcpy(table, plan.table.data(), sizeof(mpc::UnpackStream) * plan.table.size());
    for (int ch = 0; ch < 3; ++ch)
        for (int i = 0; i < K; ++i) quant[ch * K + i] = static_cast<double>(s.quant[ch][i]);
    h_flags[0] = h_flags[1] = -1;
    char* dbase = slot.dev.data();
    upload_layout(dbase);                                           // counts, coded, table, quant: their device copies now
    device_layout(dbase);
    if (q.d_rgb) d_pixels = q.d_rgb[f];
    stamps[0] = trace_ms();
    hipStream_t st = slot.stream;
    if (trace) HIP_TRY(hipEventRecord(slot.stamp[0], st));
    HIP_TRY(hipMemsetAsync(ua.error, 0, 2 * sizeof(int), st));
    HIP_TRY(hipMemcpyAsync(dbase, hbase, upload_bytes, hipMemcpyHostToDevice, st));
    if (trace) HIP_TRY(hipEventRecord(slot.stamp[1], st));
    ua.coded = coded;
    ua.streams = table;
    if (const int e = mpc::launch_unpack(ua, st); e != 0) return launch_failed(e);
    if (trace) HIP_TRY(hipEventRecord(slot.stamp[2], st));
    sa.counts = counts;
    sa.symbols = ua.symbols;
    if (const int e = mpc::launch_stream_gather(sa, d_choices, st); e != 0) return launch_failed(e);
    if (const mpc_status ds = decode_tiles_on_device(c, counts, d_choices, quant, K, s.width, s.height, d_pixels, ua.error + 1, st);
        ds != MPC_OK)
        return ds;
    if (trace) HIP_TRY(hipEventRecord(slot.stamp[3], st));
    HIP_TRY(hipMemcpyAsync(h_flags, ua.error, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    if (!q.d_rgb) HIP_TRY(hipMemcpyAsync(hbase, d_pixels, px, hipMemcpyDeviceToHost, st));    // the upload has left the buffer: stream order
    if (trace) HIP_TRY(hipEventRecord(slot.stamp[4], st));
    HIP_TRY(hipEventRecord(slot.done, st));
    HIP_TRY(hipEventSynchronize(slot.done));                        // this frame's work only: no other context's, no other slot's
    stamps[1] = trace_ms();
    if (h_flags[0] != 0 || h_flags[1] != 0) return fail(MPC_ERR_BITSTREAM, "Invalid bitstream");
    if (!q.d_rgb) {
        uint8_t* out = static_cast<uint8_t*>(std::malloc(px ? px : 1));
        if (!out) return fail(MPC_ERR_ALLOC, "out of memory");
        const size_t piece = pooled ? ((px + 15) / 16 + 4095) & ~static_cast<size_t>(4095) : px;
        const auto copy = [&](int k) {
            const size_t lo = piece * static_cast<size_t>(k), hi = std::min(px, lo + piece);
            std::memcpy(out + lo, hbase + lo, hi - lo);
        };
        if (pooled && px) mpc::parallel_jobs(static_cast<int>((px + piece - 1) / piece), copy);
        else if (px) copy(0);                                       // the frames' copies run side by side on the call's threads
        q.rgb[f] = out;
    }
    q.width[f] = s.width;
    q.height[f] = s.height;
    stamps[2] = trace_ms();
    return MPC_OK;
}

void trace_frame(int f, int slot_index, DecodeSlot& slot, const double host[6]) {
    float dev[4] = {};
    for (int k = 0; k < 4; ++k) (void)hipEventElapsedTime(&dev[k], slot.stamp[k], slot.stamp[k + 1]);
    std::fprintf(stderr,
                 "[trace] decode frame %d slot %d: parse %.2f ms | wait for the slot %.2f | staged %.2f | on the device %.2f (upload %.2f, "
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
        mpc_status st = guarded([&]() -> mpc_status {
            if (q.failed_before(f)) return MPC_OK;
            HIP_TRY(hipSetDevice(c->device));
            if (!mpc::read_compressed_coded(q.bytes[f], q.nbytes[f], s)) return fail(MPC_ERR_BITSTREAM, "Invalid input data");
            if (s.block_size != c->block_size)
                return fail(MPC_ERR_ARGUMENT, "stream block size %d, context block size %d", s.block_size, c->block_size);
            for (uint16_t length : s.lengths)
                if (length > s.K) return fail(MPC_ERR_BITSTREAM, "Invalid bitstream");
            if (q.d_rgb && static_cast<size_t>(s.width) * s.height * 3 > q.capacity[f])
                return fail(MPC_ERR_ARGUMENT, "capacity %zu for a frame of %dx%d", q.capacity[f], s.width, s.height);
            if (!plan_unpack(s.K, [&](int i) { return static_cast<unsigned long long>(s.codes[i].size()); }, s.packed.data(), nullptr,
                             s.expect.data(), plan))
                return fail(MPC_ERR_BITSTREAM, "Invalid bitstream");
            return MPC_OK;
        });
        host[1] = trace_ms();
        // The slot is taken in frame order whatever became of the parse: the frames behind count this slot's uses.
        const int slot_index = f % q.slots;
        {
            std::unique_lock<std::mutex> hold(q.lock);
            q.turn.wait(hold, [&] { return q.slot_uses[slot_index] == f / q.slots; });
        }
        host[2] = trace_ms();
        bool ran = false;
        if (st == MPC_OK && !q.failed_before(f)) {
            st = guarded([&]() -> mpc_status { return frame_on_slot(q, f, *c->dec[slot_index], s, plan, host + 3); });
            ran = st == MPC_OK;
            if (!ran) (void)hipStreamSynchronize(c->dec[slot_index]->stream);      // nothing of this frame is left on the slot's stream
        }
        if (ran && q.tuning.trace) trace_frame(f, slot_index, *c->dec[slot_index], host);
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

mpc_status decode_sequence(mpc_context* c, const uint8_t* const* bytes, const size_t* nbytes, int n_frames, uint8_t** rgb,
                           uint8_t* const* d_rgb, const size_t* capacity, int* width, int* height) {
    if (!c || !bytes || !nbytes || !width || !height || (!rgb && !d_rgb) || (d_rgb && !capacity)) return fail(MPC_ERR_ARGUMENT, "null argument");
    if (n_frames < 1) return fail(MPC_ERR_ARGUMENT, "n_frames must be at least 1");
    if (c->device < 0) return fail(MPC_ERR_NO_DEVICE, "context was created without a device; there is no CPU fallback");
    for (int f = 0; f < n_frames; ++f)
        if (!bytes[f] || (d_rgb && !d_rgb[f])) return fail(MPC_ERR_ARGUMENT, "frame %d: null argument", f);
    if (d_rgb)                                                      // before anything is enqueued; a header that does not parse fails in its turn
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
    q.slots = mpc_context::kDecodeSlots;
    q.bytes = bytes;
    q.nbytes = nbytes;
    q.rgb = rgb;
    q.d_rgb = d_rgb;
    q.capacity = capacity;
    q.width = width;
    q.height = height;
    if (const mpc_status ss = ensure_slots(c, q.slots); ss != MPC_OK) return ss;
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
    return fail(q.failed_status, "frame %d: %s", q.failed_frame, q.failed_text.c_str());
}

}  // namespace

extern "C" {

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

mpc_status mpc_unpack_symbol_streams_device(mpc_context* c, int K, const uint16_t* coded, const unsigned long long* coded_off,
                                            const uint8_t* is_packed, const unsigned long long* expect, uint16_t** symbols,
                                            size_t* n_symbols) {
    return guarded([&]() -> mpc_status {
        if (!c || !coded_off || !is_packed || !expect || !symbols || !n_symbols) return fail(MPC_ERR_ARGUMENT, "null argument");
        if (K < 1 || K > MPC_MAX_K) return fail(MPC_ERR_ARGUMENT, "K = %d", K);
        if (c->device < 0) return fail(MPC_ERR_NO_DEVICE, "context was created without a device; there is no CPU fallback");
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
        uint16_t* up_coded;
        mpc::UnpackStream* up_table;
        auto upload_layout = [&](char* base) {
            Carve cv{base};
            up_coded = cv.take<uint16_t>(plan.n_coded + 2);
            up_table = cv.take<mpc::UnpackStream>(plan.table.size());
            return cv.at;
        };
        const size_t upload_bytes = upload_layout(nullptr);
        mpc::UnpackArgs ua{};
        auto device_layout = [&](char* base) {
            Carve cv{base};
            cv.at = upload_bytes;
            carve_unpack(cv, plan, K, &ua);
            return cv.at;
        };
        const size_t out_bytes = sizeof(uint16_t) * plan.n_symbols;
        constexpr size_t kHead = 256;
        if (const mpc_status gs = slot.pinned.reserve(kHead + std::max(upload_bytes, Carve::up(out_bytes)), "pinned decode staging"); gs != MPC_OK)
            return gs;
        if (const mpc_status gs = slot.dev.reserve(device_layout(nullptr), "device decode staging"); gs != MPC_OK) return gs;
        char* hbase = slot.pinned.data() + kHead;
        int* h_flags = reinterpret_cast<int*>(slot.pinned.data());
        upload_layout(hbase);
        if (plan.n_coded) std::memcpy(up_coded, coded, sizeof(uint16_t) * plan.n_coded);
        std::memcpy(up_table, plan.table.data(), sizeof(mpc::UnpackStream) * plan.table.size());
        h_flags[0] = -1;
        char* dbase = slot.dev.data();
        upload_layout(dbase);
        device_layout(dbase);
        ua.coded = up_coded;
        ua.streams = up_table;
        hipStream_t st = slot.stream;
        HIP_TRY(hipMemsetAsync(ua.error, 0, 2 * sizeof(int), st));
        HIP_TRY(hipMemcpyAsync(dbase, hbase, upload_bytes, hipMemcpyHostToDevice, st));
        if (const int e = mpc::launch_unpack(ua, st); e != 0) return launch_failed(e);
        HIP_TRY(hipMemcpyAsync(h_flags, ua.error, sizeof(int), hipMemcpyDeviceToHost, st));
        if (out_bytes) HIP_TRY(hipMemcpyAsync(hbase, ua.symbols, out_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(slot.done, st));
        HIP_TRY(hipEventSynchronize(slot.done));
        if (h_flags[0] != 0) return fail(MPC_ERR_BITSTREAM, "Invalid bitstream");
        uint16_t* out = static_cast<uint16_t*>(std::malloc(out_bytes ? out_bytes : 2));
        if (!out) return fail(MPC_ERR_ALLOC, "out of memory");
        if (out_bytes) std::memcpy(out, hbase, out_bytes);
        *symbols = out;
        *n_symbols = plan.n_symbols;
        return MPC_OK;
    });
}

}  // extern "C"
