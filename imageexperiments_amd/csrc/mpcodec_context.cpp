// mpcodec_context.cpp -- product: the C ABI's contexts over the host dictionary builder and the gfx950 kernels: the device
// dictionary, contexts and their quantiser tables, the pursuit launches (tile encode), kernel timing, the tuning switches.  There
// is NO CPU fallback for the hot path: without a HIP device mpc_encode_tiles* return MPC_ERR_NO_DEVICE.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "mpc_internal.h"

namespace {
thread_local char g_error[512] = "";

template <class T>
hipError_t upload(T** dst, const T* src, size_t count) {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(dst), count * sizeof(T));
    if (e != hipSuccess) return e;
    return hipMemcpy(*dst, src, count * sizeof(T), hipMemcpyHostToDevice);
}
}  // namespace

mpc_status fail(mpc_status st, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
    return st;
}

Tuning read_tuning() {
    auto env_int = [](const char* name, int fallback) {
        const char* v = std::getenv(name);
        return (v && *v) ? std::atoi(v) : fallback;
    };
    Tuning t;
    const char* path = std::getenv("MPC_PATH");
    t.steps_path = (path && std::strcmp(path, "steps") == 0) || env_int("MPC_FILTER", 1) == 0;
    t.pipes = env_int("MPC_PIPES", 0);
    const int tiles = env_int("MPC_MAX_BATCH_TILES", 0);
    if (tiles > 0) t.max_batch = 3LL * ((tiles + 255) / 256 * 256);
    t.workgroups = env_int("MPC_WORKGROUPS", 0);
    t.seq_workgroups = env_int("MPC_SEQ_WORKGROUPS", -1);
    t.lag_assembly = std::min(4, std::max(2, env_int("MPC_LAG_ASSEMBLY", 2)));
    t.lag_phase2 = std::min(5, std::max(t.lag_assembly, env_int("MPC_LAG_PHASE2", 3)));
    t.seq_group = std::min(3, std::max(0, env_int("MPC_SEQ_GROUP", 0)));
    t.single_stripes = std::min(static_cast<int>(mpc_context::kSingleStripes), env_int("MPC_SINGLE_STRIPES", 0));
    t.host_entropy = env_int("MPC_HOST_ENTROPY", 0) != 0;
    const int triples = env_int("MPC_ENTROPY_TRIPLES", 0);
    if (triples > 0 && static_cast<unsigned>(triples) < kTripleCap) t.triple_limit = static_cast<unsigned>(triples);
    t.trace = env_int("MPC_TRACE", 0) != 0;
    return t;
}

double trace_ms() {
    static const auto origin = std::chrono::steady_clock::now();
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - origin).count();
}

mpc_status GrowBuffer::reserve(size_t need, const char* what, bool* grown) {
    if (grown) *grown = false;
    if (need <= bytes) return MPC_OK;
    if (p) {
        HIP_TRY(hipDeviceSynchronize());
        release();
    }
    const hipError_t e = kind == kDevice ? hipMalloc(&p, need)
                                         : hipHostMalloc(&p, need, kind == kMapped ? hipHostMallocMapped : hipHostMallocDefault);
    if (e != hipSuccess) {
        p = nullptr;
        return fail(MPC_ERR_ALLOC, "%s of %zu bytes: %s", what, need, hipGetErrorString(e));
    }
    bytes = need;
    if (grown) *grown = true;
    return MPC_OK;
}

void GrowBuffer::release() {
    if (p) (void)(kind == kDevice ? hipFree(p) : hipHostFree(p));
    p = nullptr;
    bytes = 0;
}

void carve_stream_buffers(Carve& cv, long long tiles, int K, bool assembly, mpc::StreamArgs* sa) {
    const size_t n_tc = 3 * static_cast<size_t>(tiles);
    sa->tiles = tiles;
    sa->K = K;
    sa->block_live = cv.take<unsigned>(mpc::stream_workspace_words(tiles, K));
    sa->sizes = cv.take<unsigned>(3 * static_cast<size_t>(K));
    if (!assembly) return;
    sa->stream_off = cv.take<unsigned long long>(6 * static_cast<size_t>(K) + 1);
    sa->symbols = cv.take<uint16_t>(2 * n_tc * K);
    sa->dc_tmp = cv.take<uint16_t>(n_tc);
}

hipError_t staged_upload(int device, const uint8_t* src, uint8_t* pinned, uint8_t* dst, size_t lo, size_t hi, size_t parts,
                         hipStream_t stream) {
    const size_t chunk = std::max<size_t>(size_t(1) << 20, (((hi - lo + parts - 1) / parts) + 4095) & ~static_cast<size_t>(4095));
    const int chunks = static_cast<int>((hi - lo + chunk - 1) / chunk);
    std::atomic<int> failed{static_cast<int>(hipSuccess)};
    mpc::parallel_io_jobs(chunks, 8, [&](int k) {
        const size_t a = lo + chunk * static_cast<size_t>(k), b = std::min(hi, a + chunk);
        std::memcpy(pinned + a, src + a, b - a);
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) e = hipMemcpyAsync(dst + a, pinned + a, b - a, hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) failed.store(static_cast<int>(e));
    });
    return static_cast<hipError_t>(failed.load());
}

namespace {
std::mutex g_dicts_lock;
std::weak_ptr<DeviceDict> g_dicts[64];

// build (or share) the device residents of `dict` on `device`
hipError_t acquire_device_dict(int device, const mpc::Dictionary& dict, std::shared_ptr<DeviceDict>* out) {
    std::lock_guard<std::mutex> hold(g_dicts_lock);
    if (device < 64)
        if (std::shared_ptr<DeviceDict> have = g_dicts[device].lock()) { *out = have; return hipSuccess; }
    std::shared_ptr<DeviceDict> d = std::make_shared<DeviceDict>();
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return e;
    d->device = device;
    d->num_base = dict.num_base;
    d->detail_rows = dict.total_detail_rows();
    std::vector<double> base = mpc::base_padded(dict, 2, &d->base_rows_padded);
    const size_t det_rows = static_cast<size_t>(dict.total_detail_rows());
    // one zero row after the last: the exhaustive sweep's scalar prefetch reads one row past the rows it correlates
    std::vector<double> det((3 * det_rows + 1) * mpc::kTileN, 0.0);
    for (int ch = 0; ch < 3; ++ch)
        std::memcpy(det.data() + ch * det_rows * mpc::kTileN, dict.detail[ch].data(), det_rows * mpc::kTileN * sizeof(double));
    {   // base rows and detail rows in one allocation
        std::vector<double> all(base);
        all.insert(all.end(), det.begin(), det.end());
        e = upload(&d->d_base, all.data(), all.size());
        d->d_detail = d->d_base + base.size();
        const std::vector<float> all32(all.begin(), all.end());                                       // round to nearest
        if (e == hipSuccess) e = upload(&d->d_base32, all32.data(), all32.size());
        d->d_detail32 = d->d_base32 + base.size();
    }
    if (e == hipSuccess) e = upload(&d->d_rows, dict.block_rows.data(), dict.block_rows.size());
    if (e == hipSuccess) e = upload(&d->d_rowoff, dict.block_row_off.data(), dict.block_row_off.size());
    // split-bfloat16 filter copies in MFMA operand order (host_dictionary.h: filter_tiles, k order 1): base rows as 32 tiles of
    // 16 rows, every detail block as 4
    std::vector<uint8_t> shadow(3 * det_rows, 0);
    if (e == hipSuccess) {
        const std::vector<uint16_t> base_t = mpc::filter_tiles(dict.base.data(), dict.num_base, mpc::kBaseFilterTiles, 1);
        std::vector<uint16_t> det_t;
        det_t.reserve(3 * static_cast<size_t>(dict.num_base) * mpc::kBlockFilterTiles * mpc::kFilterTileHalves);
        for (int ch = 0; ch < 3; ++ch)
            for (int b = 0; b < dict.num_base; ++b) {
                std::vector<uint8_t> sh;
                const std::vector<uint16_t> t = mpc::filter_tiles(
                    dict.detail[ch].data() + static_cast<size_t>(dict.block_row_off[b]) * mpc::kTileN, dict.block_rows[b],
                    mpc::kBlockFilterTiles, 1, &sh);
                det_t.insert(det_t.end(), t.begin(), t.end());
                std::copy(sh.begin(), sh.end(), shadow.begin() + static_cast<size_t>(ch) * det_rows + static_cast<size_t>(dict.block_row_off[b]));
            }
        e = upload(&d->d_base_t1, base_t.data(), base_t.size());
        if (e == hipSuccess) e = upload(&d->d_detail_t1, det_t.data(), det_t.size());
    }
    if (e == hipSuccess) e = upload(&d->d_shadow, shadow.data(), shadow.size());
    if (e == hipSuccess) e = hipDeviceGetAttribute(&d->num_cus, hipDeviceAttributeMultiprocessorCount, device);
    // Gram table, built on the device
    const long long n_sel = dict.num_base + static_cast<long long>(det_rows), stride = static_cast<long long>(dict.num_base) * 64;
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d->d_gram), sizeof(float) * 3 * n_sel * stride);
    for (int ch = 0; ch < 3 && e == hipSuccess; ++ch)
        e = static_cast<hipError_t>(mpc::launch_gram(d->d_base, d->d_detail + static_cast<size_t>(ch) * det_rows * mpc::kTileN, d->d_rows,
                                                     d->d_rowoff, d->d_shadow + static_cast<size_t>(ch) * det_rows,
                                                     d->d_gram + static_cast<size_t>(ch) * n_sel * stride, dict.num_base,
                                                     static_cast<int>(n_sel), stride, nullptr));
    // persistent kernel: streams, events, queue words, per-wave scratch for one workgroup per CU
    d->workgroups = d->num_cus > 0 ? d->num_cus : 1;
    if (e == hipSuccess) e = hipEventCreateWithFlags(&d->done[0], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(d->done[0], nullptr);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d->queues), 64);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d->stats), 2 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(d->stats, 0, 2 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d->pair_p), sizeof(float) * mpc::pursuit_scratch_floats(d->workgroups));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d->pair_meta), sizeof(unsigned) * mpc::pursuit_scratch_meta(d->workgroups));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d->pair_e), sizeof(float) * mpc::pursuit_scratch_bounds(d->workgroups));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return e;
    if (device < 64) g_dicts[device] = d;
    *out = d;
    return hipSuccess;
}
}  // namespace

// device table a call quantises with: the context's, or a ring slot holding the call's override (mpc_internal.h: CallQuant)
mpc_status header_quant_device(mpc_context* c, const double* quant, hipStream_t s, CallQuant* cq) {
    const double* q = quant ? quant : c->quant.data();
    double carried[3 * MPC_MAX_K];
    for (int i = 0; i < 3 * c->K; ++i) carried[i] = static_cast<double>(mpc::header_quant(q[i]));
    return call_quant(c, carried, s, cq);
}

mpc_status call_quant(mpc_context* c, const double* quant, hipStream_t s, CallQuant* q) {
    q->d_q = c->d_quant;
    if (!quant) return MPC_OK;
    q->hold = std::unique_lock<std::mutex>(c->quant_lock);     // until ~CallQuant: take, fill, read and let go are one step per context
    const int slot = static_cast<int>(c->quant_next++ % mpc_context::kQuantSlots);
    double* table = c->d_quant_ring + static_cast<size_t>(slot) * 3 * MPC_MAX_K;
    HIP_TRY(hipStreamWaitEvent(s, c->quant_free[slot], 0));    // the slot's last reader, on whatever stream it ran, is through
    q->ctx = c;
    q->slot = slot;
    q->stream = s;
    const int err = mpc::launch_quant_table(quant, c->K, table, s);
    if (err != 0) return launch_failed(err);
    q->d_q = table;
    return MPC_OK;
}

CallQuant::~CallQuant() {
    if (slot >= 0) (void)hipEventRecord(ctx->quant_free[slot], stream);
}

mpc_status refuse_capture(void* stream) {
    if (!stream) return MPC_OK;                               // the null stream cannot be captured
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing(static_cast<hipStream_t>(stream), &status));
    if (status != hipStreamCaptureStatusNone)
        return fail(MPC_ERR_ARGUMENT, "the stream is being captured into a graph: not supported (the calls of a process share scratch that a "
                                      "replayed graph would use out of turn)");
    return MPC_OK;
}

mpc::DictDevice dict_device(const mpc_context* c) {
    mpc::DictDevice d{};
    const DeviceDict& dd = *c->dd;
    d.base = dd.d_base;
    d.num_base = c->dict.num_base;
    d.base_rows_padded = dd.base_rows_padded;
    d.detail = dd.d_detail;
    d.base32 = dd.d_base32;
    d.detail32 = dd.d_detail32;
    d.detail_rows = c->dict.total_detail_rows();
    d.block_rows = dd.d_rows;
    d.block0_rows = c->dict.block_rows.empty() ? 0 : c->dict.block_rows[0];
    d.block_row_off = dd.d_rowoff;
    return d;
}

namespace {
// how many sub-batches of a call run concurrently (measured on MI355X: 2 for a 1080p frame, 3 from ~300k
// tile-channels up, 4 for an 8K frame)
int pipes_for(const Tuning& t, long long tile_channels) {
    if (t.pipes > 0) return std::min(t.pipes, 4);
    if (tile_channels <= 3 * 4096) return 1;              // do not split what cannot fill the machine
    return tile_channels >= 1200000 ? 4 : (tile_channels >= 300000 ? 3 : 2);      // 4: an 8K frame
}
}  // namespace

// grow-only workspaces of the step-synchronous exhaustive sweeps (MPC_PATH=steps); allocation synchronises the device, so
// callers that must not call mpc_reserve() first
mpc_status ensure_workspace(mpc_context* c, const Tuning& t, long long tile_channels) {
    if (!t.steps_path) return MPC_OK;                 // the persistent kernel's scratch lives in the shared DeviceDict
    const int want_pipes = pipes_for(t, tile_channels);
    long long total = std::min(tile_channels, t.max_batch);
    long long cap = (total + want_pipes - 1) / want_pipes;
    cap = (cap + 767) / 768 * 768;                                        // whole units (3 tile-channels), whole 256-blocks
    if (cap <= c->ws_cap && static_cast<int>(c->pipes.size()) >= want_pipes) return MPC_OK;
    if (hipDeviceSynchronize() != hipSuccess) return fail(MPC_ERR_HIP, "device synchronise failed");
    if (!c->fork && hipEventCreateWithFlags(&c->fork, hipEventDisableTiming) != hipSuccess)
        return fail(MPC_ERR_HIP, "event creation failed");
    while (static_cast<int>(c->pipes.size()) < want_pipes) {
        mpc_context::Pipe p;
        if (hipStreamCreateWithFlags(&p.stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&p.done, hipEventDisableTiming) != hipSuccess)
            return fail(MPC_ERR_HIP, "stream/event creation failed");
        c->pipes.push_back(p);
    }
    if (cap < c->ws_cap) cap = c->ws_cap;
    const size_t bytes = mpc::workspace_bytes(static_cast<int>(cap), c->K);
    for (auto& p : c->pipes) {
        if (p.mem && cap == c->ws_cap) continue;          // already large enough
        if (p.mem) (void)hipFree(p.mem);
        p.mem = nullptr;
        hipError_t e = hipMalloc(&p.mem, bytes);
        if (e != hipSuccess) { c->ws_cap = 0; return fail(MPC_ERR_ALLOC, "workspace of %zu bytes: %s", bytes, hipGetErrorString(e)); }
        p.ws = mpc::carve_workspace(p.mem, static_cast<int>(cap), c->K);
    }
    c->ws_cap = static_cast<int>(cap);
    return MPC_OK;
}

// Sweep work is cut fine (8 atom ranges per 64 tile-channels, 4 row ranges per detail block) and handed to
// machine-sized persistent grids, so a step's last round is nearly full whatever the active count is.
constexpr int kBaseParts = 8;
constexpr int kRowParts = 4;

namespace {
// mpc_kernel_timing_*: the next n of the context's timing events (*ev stays null while timing is off)
hipError_t timing_events(mpc_context* c, size_t n, hipEvent_t** ev) {
    if (!c->timing) return hipSuccess;
    const size_t need = c->timing_used + n;
    while (c->timing_events.size() < need) {
        hipEvent_t e;
        if (const hipError_t err = hipEventCreate(&e); err != hipSuccess) return err;
        c->timing_events.push_back(e);
    }
    *ev = c->timing_events.data() + c->timing_used;
    c->timing_used = need;
    return hipSuccess;
}

#ifdef MPC_STAMPS
// Diagnostic builds only (tools/stamps.sh): the in-kernel phase stamps of one persistent launch, cleared before it and reported
// on stderr after it (both synchronise the stream).
constexpr int kDebugWords = 24 + 2 * 1024;

hipError_t stamps_reset(hipStream_t s, unsigned long long** debug) {
    static unsigned long long* d_debug = nullptr;
    hipError_t e = d_debug ? hipSuccess : hipMalloc(reinterpret_cast<void**>(&d_debug), kDebugWords * sizeof(unsigned long long));
    std::vector<unsigned long long> init(kDebugWords, 0ULL);
    for (int b = 0; b < 1024; ++b) init[24 + 2 * b] = ~0ULL;
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipMemcpy(d_debug, init.data(), kDebugWords * sizeof(unsigned long long), hipMemcpyHostToDevice);
    *debug = d_debug;
    return e;
}

hipError_t stamps_report(hipStream_t s, const unsigned long long* d_debug, int workgroups, int cus) {
    std::vector<unsigned long long> all(kDebugWords);
    hipError_t e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipMemcpy(all.data(), d_debug, kDebugWords * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    const unsigned long long* hst = all.data();
    unsigned long long tot = 0;
    for (int i = 0; i < 12; ++i) tot += hst[i];
    std::fprintf(stderr, "[stamps wg%d] wave-steps %llu live-lanes/step %.1f pass2-groups %llu rounds %llu exhaustive %llu | cycles/wave-step:",
                 workgroups, hst[12], hst[12] ? (double)hst[16] / hst[12] / 4.0 : 0.0, hst[13], hst[14], hst[15]);
    for (int i = 0; i < 12; ++i) std::fprintf(stderr, " %d:%.0f", i, hst[12] ? (double)hst[i] / hst[12] : 0.0);
    std::fprintf(stderr, " total %.0f | pair rounds/step %.2f items/round %.2f new pairs/step %.2f\n", hst[12] ? (double)tot / hst[12] : 0.0,
                 hst[12] ? (double)hst[17] / hst[12] : 0.0, hst[17] ? (double)hst[18] / hst[17] : 0.0, hst[12] ? (double)hst[19] / hst[12] : 0.0);
    // workgroup residency: how many workgroups are on the machine over the launch (20 slices), and per channel when its
    // first / last workgroup came and went (microseconds from the first workgroup's start; 100 MHz counter)
    const int grid = workgroups;
    unsigned long long t0 = ~0ULL, t1 = 0;
    for (int b = 0; b < grid && b < 1024; ++b) { t0 = std::min(t0, all[24 + 2 * b]); t1 = std::max(t1, all[25 + 2 * b]); }
    if (t1 > t0) {
        const double span = (double)(t1 - t0);
        double busy = 0.0;
        int slices[20] = {};
        for (int b = 0; b < grid && b < 1024; ++b) {
            busy += (double)(all[25 + 2 * b] - all[24 + 2 * b]);
            for (int k = 0; k < 20; ++k) {
                const double mid = t0 + span * (k + 0.5) / 20.0;
                if ((double)all[24 + 2 * b] <= mid && mid < (double)all[25 + 2 * b]) ++slices[k];
            }
        }
        std::fprintf(stderr, "[residency] span %.1f us, workgroup-time / (%d CUs x span) = %.3f | resident workgroups per 5 %% slice:", span / 100.0,
                     cus, busy / (span * cus));
        for (int k = 0; k < 20; ++k) std::fprintf(stderr, " %d", slices[k]);
        std::fprintf(stderr, "\n");
    }
    return hipSuccess;
}
#endif

// The persistent path (mp_pursuit.hip): ONE launch on the caller's stream runs all K steps of every tile-channel; its
// workgroups are split over the channels (a workgroup's LDS holds one channel's DetailBasis[0]).  No host synchronisation,
// no allocation.  Launches of one process are serialised on the device by a lock-ordered event chain, because they share the
// per-device scratch and queue words.  That chain is why a capturing stream is refused (refuse_capture, in front of every caller):
// the wait below would be on an event recorded outside the capture, the record behind the launch would leave done[0] a captured
// event that the next plain launch cannot wait on, and a replay takes no part in the chain at all, so it would share the queue
// words with whatever another stream launches beside it.
mpc_status run_persistent(mpc_context* c, const Tuning& t, const mpc::FrameInput& in, const mpc::Outputs& out, const double* d_quant,
                          long long total_tc, void* stream) {
    DeviceDict& d = *c->dd;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool vec = in.vec_in != nullptr;
    const long long n_tc = vec ? total_tc : total_tc / 3;
    const long long n_units = (n_tc + 15) / 16 * (vec ? 1 : 3);         // groups of 16 tile-channels, all channels
    if (n_tc >= (1LL << 31)) return fail(MPC_ERR_ARGUMENT, "batch too large");
    // One workgroup fits a CU (its LDS holds the dictionary); its waves start on luma and move on to the chroma channels as the
    // queues run dry (mp_pursuit.hip: channel switch), so a small frame spreads over the channels by itself.
    const int per_wg = mpc::pursuit_units_per_workgroup();
    int workgroups = static_cast<int>(std::min<long long>((n_units + per_wg - 1) / per_wg, d.workgroups));
    if (const int limit = c->seq_workgroups.load(std::memory_order_relaxed); limit > 0) workgroups = std::min(workgroups, limit);
    if (const int limit = c->user_workgroups.load(std::memory_order_relaxed); limit > 0) workgroups = std::min(workgroups, limit);
    if (t.workgroups > 0) workgroups = std::min(t.workgroups, d.workgroups);
    std::lock_guard<std::mutex> hold(d.launch_lock);
    HIP_TRY(hipStreamWaitEvent(s, d.done[0], 0));             // the previous launch of this process (any stream) has drained
    HIP_TRY(hipMemsetAsync(d.queues, 0, 3 * sizeof(unsigned), s));
    const long long n_sel = d.num_base + d.detail_rows, stride = static_cast<long long>(d.num_base) * 64;
    mpc::PursuitArgs a{};
    a.base = d.d_base;
    a.base32 = d.d_base32;

    a.fast = c->fast ? 1 : 0;
    a.base_tiles = d.d_base_t1;
    for (int ch = 0; ch < 3; ++ch) {
        a.detail[ch] = d.d_detail + static_cast<size_t>(ch) * d.detail_rows * mpc::kTileN;
        a.detail32[ch] = d.d_detail32 + static_cast<size_t>(ch) * d.detail_rows * mpc::kTileN;
        a.block_tiles[ch] = d.d_detail_t1 + static_cast<size_t>(ch) * d.num_base * mpc::kBlockFilterTiles * mpc::kFilterTileHalves;
        a.gram[ch] = d.d_gram + static_cast<size_t>(ch) * n_sel * stride;
        a.n_tc[ch] = vec ? (ch == in.vec_channel ? n_tc : 0) : n_tc;
    }
    a.pair_p = d.pair_p;
    a.pair_meta = d.pair_meta;
    a.pair_e = d.pair_e;
    a.workgroups = workgroups;
    a.gram_stride = stride;
    a.block_rows = d.d_rows;
    a.block_row_off = d.d_rowoff;
    a.quant = d_quant;
    a.K = c->K;
    a.num_base = d.num_base;
    a.rows0 = c->dict.block_rows.empty() ? 0 : c->dict.block_rows[0];
    for (int f = 0; f < mpc::kFrameTable; ++f) {               // the strided form: one base, records back to back
        a.frame_rgb[f] = in.rgb;
        a.frame_first[f] = 0;
    }
    a.width = in.width;
    a.height = in.height;
    a.row_stride = in.row_stride;
    a.frame_stride = in.frame_stride;
    a.tile_row_begin = in.tile_row_begin;
    a.tile_rows = in.tile_rows;
    a.tiles_x = in.tiles_x;
    a.out_tile_rows = in.out_tile_rows;
    a.rgb_aligned8 = (reinterpret_cast<uintptr_t>(in.rgb) % 8 == 0 && in.row_stride % 8 == 0 && (in.frames <= 1 || in.frame_stride % 8 == 0)) ? 1 : 0;
    if (in.table.n > 0) {                                     // frames that lie anywhere: a base and a record offset each
        a.frame_stride = 0;
        a.rgb_aligned8 = in.row_stride % 8 == 0 ? 1 : 0;
        const long long tiles_per_frame = static_cast<long long>(in.tiles_x) * in.tile_rows;
        for (int f = 0; f < mpc::kFrameTable; ++f) {
            const int k = f < in.table.n ? f : 0;
            a.frame_rgb[f] = in.table.rgb[k];
            a.frame_first[f] = static_cast<int>(in.table.first[k] - f * tiles_per_frame);
            if (reinterpret_cast<uintptr_t>(in.table.rgb[k]) % 8 != 0) a.rgb_aligned8 = 0;   // one frame off the 8-byte grid: all read bytes
        }
    }
    a.vec_in = in.vec_in;
    a.vec_channel = in.vec_channel;
    a.queue = d.queues;
    a.out = out;
    a.stats = d.stats;
    hipEvent_t* ev = nullptr;
    HIP_TRY(timing_events(c, 2, &ev));
    if (ev) HIP_TRY(hipEventRecord(ev[0], s));
#ifdef MPC_STAMPS
    HIP_TRY(stamps_reset(s, &a.debug));
#endif
    const int err = mpc::launch_pursuit(a, s);
    if (err != 0) return launch_failed(err);
    if (ev) HIP_TRY(hipEventRecord(ev[1], s));
    HIP_TRY(hipEventRecord(d.done[0], s));
#ifdef MPC_STAMPS
    HIP_TRY(stamps_report(s, a.debug, a.workgroups, d.workgroups));
#endif
    return MPC_OK;
}

mpc_status run_pursuit(mpc_context* c, const Tuning& t, const mpc::FrameInput& in, const mpc::Outputs& out, const double* d_quant,
                       long long total_tc, void* stream) {
    // MPC_PATH=steps / MPC_FILTER=0: the step-synchronous exhaustive double sweeps of mp_kernels.hip (the product's own
    // cross-check); default: the persistent kernel
    if (!t.steps_path) return run_persistent(c, t, in, out, d_quant, total_tc, stream);
    if (in.table.n > 0) return fail(MPC_ERR_ARGUMENT, "a frame table runs on the persistent kernel only (unset MPC_PATH / MPC_FILTER)");
    if (c->fast) return fail(MPC_ERR_ARGUMENT, "the float flavour runs on the persistent kernel only (unset MPC_PATH / MPC_FILTER)");
    mpc_status st = ensure_workspace(c, t, total_tc);
    if (st != MPC_OK) return st;
    const mpc::DictDevice dict = dict_device(c);
    hipStream_t caller = static_cast<hipStream_t>(stream);
    // sub-batch size: an even share per pipe (whole units), at most the workspace capacity
    const long long npipes = pipes_for(t, total_tc);
    long long share = (total_tc + npipes - 1) / npipes;
    share = (share + 767) / 768 * 768;
    if (share > c->ws_cap) share = c->ws_cap;
    HIP_TRY(hipEventRecord(c->fork, caller));
    size_t used_pipes = 0;
    long long index = 0;
    for (long long begin = 0; begin < total_tc; begin += share, ++index) {
        const long long n = (total_tc - begin < share) ? total_tc - begin : share;
        auto& pipe = c->pipes[static_cast<size_t>(index % npipes)];
        if (index < npipes) {
            HIP_TRY(hipStreamWaitEvent(pipe.stream, c->fork, 0));
            ++used_pipes;
        }
        hipEvent_t* events = nullptr;
        HIP_TRY(timing_events(c, 2 * static_cast<size_t>(c->K), &events));
        const int err = mpc::enqueue_pursuit(dict, pipe.ws, in, out, d_quant, c->K, begin, static_cast<int>(n), kBaseParts, kRowParts,
                                             c->max_waves, pipe.stream, reinterpret_cast<void**>(events));
        if (err != 0) return launch_failed(err);
    }
    for (size_t i = 0; i < used_pipes; ++i) {
        HIP_TRY(hipEventRecord(c->pipes[i].done, c->pipes[i].stream));
        HIP_TRY(hipStreamWaitEvent(caller, c->pipes[i].done, 0));
    }
    return MPC_OK;
}

// What every tile encoder refuses before it touches a frame, the caller's or its own: context, pointers, geometry, stride, tile
// rows, batch.  The host form checks with this BEFORE it reads the caller's memory, the device forms before anything is enqueued.
mpc_status check_encode_args(const mpc_context* c, const uint8_t* rgb, int frames, size_t frame_stride, int width, int height,
                             size_t row_stride, int tile_row_begin, int tile_row_end, const uint16_t* counts,
                             const mpc_basis_choice* choices) {
    if (!c) return fail(MPC_ERR_ARGUMENT, "null context");
    if (c->device < 0) return no_device();
    if (!rgb || !counts || !choices) return fail(MPC_ERR_ARGUMENT, "null buffer");
    if (width < 1 || height < 1 || row_stride < static_cast<size_t>(3) * width)
        return fail(MPC_ERR_ARGUMENT, "bad geometry %dx%d stride %zu", width, height, row_stride);
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    if (tile_row_begin < 0 || tile_row_end > tiles_y || tile_row_begin >= tile_row_end)
        return fail(MPC_ERR_ARGUMENT, "tile rows [%d,%d) outside 0..%d", tile_row_begin, tile_row_end, tiles_y);
    if (frames < 1 || (frames > 1 && frame_stride < row_stride * static_cast<size_t>(height)))
        return fail(MPC_ERR_ARGUMENT, "bad batch: %d frames, stride %zu", frames, frame_stride);
    const long long tiles = static_cast<long long>(tiles_x) * (tile_row_end - tile_row_begin) * frames;
    if (tiles * 3 >= (1LL << 31)) return fail(MPC_ERR_ARGUMENT, "batch too large");
    return MPC_OK;
}
}  // namespace

// whole_frame_order: the records go where one launch over the whole frame would put them (FrameInput::out_tile_rows) and the
// caller has zeroed d_choices for the whole frame (stripes of one frame encoded one by one, encode_sequence's single frames)
// table: the frames of the launch lie anywhere and so do their records in d_counts / d_choices (mpc::FrameTable; d_rgb and
// frame_stride are the first frame's and 0); the records beyond a tile-channel's count are left as they are, not zeroed
mpc_status encode_batch_device(mpc_context* c, const Tuning& t, const uint8_t* d_rgb, int frames, size_t frame_stride, int width,
                               int height, size_t row_stride, int tile_row_begin, int tile_row_end, const double* quant,
                               uint16_t* d_counts, mpc_basis_choice* d_choices, double* d_energy, uint32_t* d_swept, void* stream,
                               bool whole_frame_order, const mpc::FrameTable* table) {
    if (table) {
        if (table->n != frames || frames > mpc::kFrameTable || whole_frame_order) return fail(MPC_ERR_ARGUMENT, "bad frame table");
        for (int f = 0; f < frames; ++f)
            if (!table->rgb[f] || table->first[f] < 0 || table->first[f] > ((1LL << 31) - 1) / 3 - (width + 7) / 8 * static_cast<long long>((height + 7) / 8))
                return fail(MPC_ERR_ARGUMENT, "bad frame table");
        frame_stride = row_stride * static_cast<size_t>(height);  // not read by the kernel; keeps the batch check below meaningful
    }
    if (const mpc_status as = check_encode_args(c, d_rgb, frames, frame_stride, width, height, row_stride, tile_row_begin, tile_row_end,
                                                d_counts, d_choices);
        as != MPC_OK)
        return as;
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    const long long tiles = static_cast<long long>(tiles_x) * (tile_row_end - tile_row_begin) * frames;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(c->device));
    if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
    CallQuant cq;
    if (const mpc_status qs = call_quant(c, quant, s, &cq); qs != MPC_OK) return qs;
    if (!whole_frame_order && !table) HIP_TRY(hipMemsetAsync(d_choices, 0, sizeof(mpc_basis_choice) * tiles * 3 * c->K, s));
    mpc::FrameInput in{};
    if (table) in.table = *table;
    in.rgb = d_rgb;
    in.width = width;
    in.height = height;
    in.row_stride = static_cast<long long>(row_stride);
    in.frames = frames;
    in.frame_stride = static_cast<long long>(frame_stride);
    in.tile_row_begin = tile_row_begin;
    in.tile_rows = tile_row_end - tile_row_begin;
    in.tiles_x = tiles_x;
    in.out_tile_rows = whole_frame_order ? tiles_y : 0;
    in.vec_in = nullptr;
    in.vec_channel = 0;
    mpc::Outputs out{};
    out.counts = d_counts;
    out.choices = reinterpret_cast<uint32_t*>(d_choices);
    out.energy = d_energy;
    out.swept = d_swept;
    return run_pursuit(c, t, in, out, cq.d_q, tiles * 3, stream);
}

extern "C" {

const char* mpc_version(void) { return "mpcodec 0.1 (gfx950)"; }
const char* mpc_last_error(void) { return g_error; }
void mpc_set_error_text(const char* text) { std::snprintf(g_error, sizeof g_error, "%s", text ? text : ""); }

mpc_status mpc_context_create(int K, int block_size, double bpp, int device, mpc_context** out) {
    return guarded([&]() -> mpc_status {
    if (!out) return fail(MPC_ERR_ARGUMENT, "out is null");
    *out = nullptr;
    if (K < 1 || K > MPC_MAX_K) return fail(MPC_ERR_ARGUMENT, "K=%d out of range 1..%d", K, MPC_MAX_K);
    if (block_size < 1 || block_size > 8) return fail(MPC_ERR_ARGUMENT, "block size %d out of range 1..8", block_size);
    if (device >= 0 && block_size != 8)
        return fail(MPC_ERR_ARGUMENT, "the device path implements 8x8 tiles only (got %d)", block_size);
    mpc_context* c = new (std::nothrow) mpc_context;
    if (!c) return fail(MPC_ERR_ALLOC, "out of memory");
    try {
        c->K = K;
        c->block_size = block_size;
        c->bpp = bpp;
        c->dict = mpc::build_dictionary(block_size);
        c->quant.resize(3 * static_cast<size_t>(K));
        mpc::quantisation_tables(K, block_size, bpp, c->quant.data());
    } catch (const std::exception& e) {
        delete c;
        return fail(MPC_ERR_ARGUMENT, "%s", e.what());
    }
    c->device = device;
    if (device >= 0) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device) {
            delete c;
            return fail(MPC_ERR_NO_DEVICE, "HIP device %d not available (%d devices visible)", device, ndev);
        }
        hipError_t e = acquire_device_dict(device, c->dict, &c->dd);
        if (e == hipSuccess) e = upload(&c->d_quant, c->quant.data(), c->quant.size());
        if (e == hipSuccess)
            e = hipMalloc(reinterpret_cast<void**>(&c->d_quant_ring), sizeof(double) * mpc_context::kQuantSlots * 3 * MPC_MAX_K);
        for (int k = 0; k < mpc_context::kQuantSlots && e == hipSuccess; ++k)
            e = hipEventCreateWithFlags(&c->quant_free[k], hipEventDisableTiming);
        if (e != hipSuccess) {
            mpc_context_destroy(c);
            return fail(MPC_ERR_HIP, "device setup failed: %s", hipGetErrorString(e));
        }
        (void)hipDeviceGetAttribute(&c->num_cus, hipDeviceAttributeMultiprocessorCount, device);
        c->max_waves = 12 * c->num_cus;
    }
    *out = c;
    return MPC_OK;
    });
}

void mpc_context_destroy(mpc_context* c) {
    if (!c) return;
    if (c->device >= 0) {
        (void)hipSetDevice(c->device);
        (void)hipFree(c->d_quant);
        (void)hipFree(c->d_quant_ring);
        for (hipEvent_t e : c->quant_free)
            if (e) (void)hipEventDestroy(e);
        (void)hipFree(c->d_flag);
        (void)hipFree(c->d_crop_flag);
        if (c->compose_side) (void)hipStreamDestroy(c->compose_side);
        if (c->budget_stream) (void)hipStreamDestroy(c->budget_stream);
        if (c->seq_up) (void)hipStreamDestroy(c->seq_up);
        if (c->seq_compute) (void)hipStreamDestroy(c->seq_compute);
        for (hipStream_t sd : c->seq_down)
            if (sd) (void)hipStreamDestroy(sd);
        for (auto& slot : c->seq_events)
            for (hipEvent_t e : slot)
                if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : c->seq_pursuit_done)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : c->seq_stripe_up)
            if (e) (void)hipEventDestroy(e);
        for (auto& p : c->pipes) {
            if (p.mem) (void)hipFree(p.mem);
            if (p.stream) (void)hipStreamDestroy(p.stream);
            if (p.done) (void)hipEventDestroy(p.done);
        }
        if (c->fork) (void)hipEventDestroy(c->fork);
        for (hipEvent_t e : c->timing_events) (void)hipEventDestroy(e);
        if (c->timing_ref) (void)hipEventDestroy(c->timing_ref);
    }
    delete c;                         // the grow-only buffers and the container jobs free themselves
}

int mpc_context_K(const mpc_context* c) { return c ? c->K : 0; }
int mpc_context_block_size(const mpc_context* c) { return c ? c->block_size : 0; }
int mpc_context_num_base(const mpc_context* c) { return c ? c->dict.num_base : 0; }
int mpc_context_detail_rows(const mpc_context* c) { return c ? c->dict.total_detail_rows() : 0; }
int mpc_context_device(const mpc_context* c) { return c ? c->device : -1; }
int mpc_context_max_waves(const mpc_context* c) { return c ? c->max_waves : 0; }

mpc_status mpc_context_set_tile_encode_workgroups(mpc_context* c, int workgroups) {
    if (!c || workgroups < 0) return fail(MPC_ERR_ARGUMENT, "bad argument");
    std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
    c->user_workgroups = workgroups;
    return MPC_OK;
}

mpc_status mpc_context_set_fast(mpc_context* c, int on) {
    if (!c) return fail(MPC_ERR_ARGUMENT, "null context");
    std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
    c->fast = on != 0;
    return MPC_OK;
}
int mpc_context_is_fast(const mpc_context* c) { return c && c->fast ? 1 : 0; }

mpc_status mpc_context_get_quant(const mpc_context* c, double* quant) {
    if (!c || !quant) return fail(MPC_ERR_ARGUMENT, "null argument");
    std::memcpy(quant, c->quant.data(), c->quant.size() * sizeof(double));
    return MPC_OK;
}

mpc_status mpc_context_set_quant(mpc_context* c, const double* quant) {
    if (!c || !quant) return fail(MPC_ERR_ARGUMENT, "null argument");
    std::memcpy(c->quant.data(), quant, c->quant.size() * sizeof(double));
    if (c->device >= 0) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipMemcpy(c->d_quant, quant, c->quant.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    return MPC_OK;
}

mpc_status mpc_context_get_dictionary(const mpc_context* c, double* base, int32_t* block_rows, double* dy, double* du,
                                      double* dv) {
    if (!c) return fail(MPC_ERR_ARGUMENT, "null context");
    if (base) std::memcpy(base, c->dict.base.data(), c->dict.base.size() * sizeof(double));
    if (block_rows) std::memcpy(block_rows, c->dict.block_rows.data(), c->dict.block_rows.size() * sizeof(int32_t));
    double* det[3] = {dy, du, dv};
    for (int ch = 0; ch < 3; ++ch)
        if (det[ch]) std::memcpy(det[ch], c->dict.detail[ch].data(), c->dict.detail[ch].size() * sizeof(double));
    return MPC_OK;
}

mpc_status mpc_encode_batch_device(mpc_context* c, const uint8_t* d_rgb, int frames, size_t frame_stride, int width,
                                   int height, size_t row_stride, int tile_row_begin, int tile_row_end,
                                   const double* quant, uint16_t* d_counts, mpc_basis_choice* d_choices,
                                   double* d_energy, uint32_t* d_swept, int waves, void* stream) {
    (void)waves;
    return encode_batch_device(c, read_tuning(), d_rgb, frames, frame_stride, width, height, row_stride, tile_row_begin, tile_row_end,
                               quant, d_counts, d_choices, d_energy, d_swept, stream, false);
}

mpc_status mpc_encode_tiles_device(mpc_context* c, const uint8_t* d_rgb, int width, int height, size_t row_stride,
                                   int tile_row_begin, int tile_row_end, const double* quant, uint16_t* d_counts,
                                   mpc_basis_choice* d_choices, double* d_energy, uint32_t* d_swept, int waves,
                                   void* stream) {
    return mpc_encode_batch_device(c, d_rgb, 1, 0, width, height, row_stride, tile_row_begin, tile_row_end, quant,
                                   d_counts, d_choices, d_energy, d_swept, waves, stream);
}

// upload, pursuit, download through the context's staging area: image | counts | records | energy | swept
mpc_status mpc_encode_tiles(mpc_context* c, const uint8_t* rgb, int width, int height, size_t row_stride,
                            int tile_row_begin, int tile_row_end, const double* quant, uint16_t* counts,
                            mpc_basis_choice* choices, double* energy, uint32_t* swept) {
    // refused before the caller's memory is read
    if (const mpc_status as = check_encode_args(c, rgb, 1, 0, width, height, row_stride, tile_row_begin, tile_row_end, counts, choices);
        as != MPC_OK)
        return as;
    const Tuning t = read_tuning();
    std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
    HIP_TRY(hipSetDevice(c->device));
    const int tiles_x = (width + 7) / 8;
    const long long tiles = static_cast<long long>(tiles_x) * (tile_row_end - tile_row_begin);
    // the bytes the frame occupies: its last row ends with its last pixel, not with a full stride (a view of a larger image
    // that ends in the parent's last row has nothing behind it)
    const size_t img_bytes = static_cast<size_t>(height - 1) * row_stride + static_cast<size_t>(3) * width;
    const size_t n_tc = static_cast<size_t>(tiles) * 3;
    uint8_t* d_rgb;
    uint16_t* d_counts;
    mpc_basis_choice* d_choices;
    double* d_energy;
    uint32_t* d_swept;
    auto layout = [&](char* base) {
        Carve cv{base};
        d_rgb = cv.take<uint8_t>(img_bytes);
        d_counts = cv.take<uint16_t>(n_tc);
        d_choices = cv.take<mpc_basis_choice>(n_tc * c->K);
        d_energy = cv.take<double>(n_tc);
        d_swept = cv.take<uint32_t>(n_tc);
        return cv.at;
    };
    if (const mpc_status gs = c->stage.reserve(layout(nullptr), "staging"); gs != MPC_OK) return gs;
    layout(c->stage.data());
    HIP_TRY(hipMemcpy(d_rgb, rgb, img_bytes, hipMemcpyHostToDevice));
    const mpc_status st = encode_batch_device(c, t, d_rgb, 1, 0, width, height, row_stride, tile_row_begin, tile_row_end, quant, d_counts,
                                              d_choices, d_energy, d_swept, nullptr, false);
    if (st != MPC_OK) return st;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(counts, d_counts, sizeof(uint16_t) * n_tc, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(choices, d_choices, sizeof(mpc_basis_choice) * n_tc * c->K, hipMemcpyDeviceToHost));
    if (energy) HIP_TRY(hipMemcpy(energy, d_energy, sizeof(double) * n_tc, hipMemcpyDeviceToHost));
    if (swept) HIP_TRY(hipMemcpy(swept, d_swept, sizeof(uint32_t) * n_tc, hipMemcpyDeviceToHost));
    return MPC_OK;
}

mpc_status mpc_histogram_device(mpc_context* c, const uint16_t* d_counts, const mpc_basis_choice* d_choices,
                                long long tiles, uint32_t* d_hist, void* stream) {
    if (!c) return fail(MPC_ERR_ARGUMENT, "null context");
    if (c->device < 0) return fail(MPC_ERR_NO_DEVICE, "context was created without a device");
    if (!d_counts || !d_choices || !d_hist || tiles < 1) return fail(MPC_ERR_ARGUMENT, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
    mpc::HistParams h{};
    h.counts = d_counts;
    h.choices = reinterpret_cast<const uint32_t*>(d_choices);
    h.tiles = tiles;
    h.K = c->K;
    h.hist = d_hist;
    const int err = mpc::launch_histogram(h, stream);
    if (err != 0) return launch_failed(err);
    return MPC_OK;
}

mpc_status mpc_calc_mp_batch(mpc_context* c, int channel, const double* quant_k, const double* inputs, int count,
                             mpc_basis_choice* choices, uint16_t* counts, double* energy, uint32_t* swept) {
    if (!c) return fail(MPC_ERR_ARGUMENT, "null context");
    if (c->device < 0) return no_device();
    if (channel < 0 || channel > 2 || !inputs || !choices || !counts || count < 1)
        return fail(MPC_ERR_ARGUMENT, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    const int K = c->K;
    std::vector<double> q(c->quant);
    if (quant_k) std::memcpy(q.data() + static_cast<size_t>(channel) * K, quant_k, sizeof(double) * K);
    DeviceTemp d_in, d_counts, d_choices, d_energy, d_swept, d_q;
    HIP_TRY(hipMalloc(&d_in.p, sizeof(double) * 64 * count));
    HIP_TRY(hipMalloc(&d_counts.p, sizeof(uint16_t) * count));
    HIP_TRY(hipMalloc(&d_choices.p, sizeof(uint32_t) * count * K));
    HIP_TRY(hipMalloc(&d_energy.p, sizeof(double) * count));
    HIP_TRY(hipMalloc(&d_swept.p, sizeof(uint32_t) * count));
    HIP_TRY(hipMalloc(&d_q.p, sizeof(double) * 3 * K));
    HIP_TRY(hipMemcpy(d_in.p, inputs, sizeof(double) * 64 * count, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_q.p, q.data(), sizeof(double) * 3 * K, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_choices.p, 0, sizeof(uint32_t) * count * K));
    mpc::FrameInput in{};
    in.vec_in = static_cast<const double*>(d_in.p);
    in.vec_channel = channel;
    in.frames = 1;
    mpc::Outputs out{};
    out.counts = static_cast<uint16_t*>(d_counts.p);
    out.choices = static_cast<uint32_t*>(d_choices.p);
    out.energy = static_cast<double*>(d_energy.p);
    out.swept = static_cast<uint32_t*>(d_swept.p);
    if (const mpc_status st = run_pursuit(c, read_tuning(), in, out, static_cast<const double*>(d_q.p), count, nullptr); st != MPC_OK)
        return st;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(counts, d_counts.p, sizeof(uint16_t) * count, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(choices, d_choices.p, sizeof(uint32_t) * count * K, hipMemcpyDeviceToHost));
    if (energy) HIP_TRY(hipMemcpy(energy, d_energy.p, sizeof(double) * count, hipMemcpyDeviceToHost));
    if (swept) HIP_TRY(hipMemcpy(swept, d_swept.p, sizeof(uint32_t) * count, hipMemcpyDeviceToHost));
    return MPC_OK;
}

// live timing of the dominant kernel (mp_pursuit_kernel; mp_base_kernel with MPC_PATH=steps) with HIP events on the launch stream
void mpc_kernel_timing_enable(mpc_context* c, int on) {
    if (!c) return;
    c->timing = on != 0;
    c->timing_used = 0;
    if (c->timing && c->device >= 0) {
        (void)hipSetDevice(c->device);
        (void)hipDeviceSynchronize();
        if (c->dd) (void)hipMemset(c->dd->stats, 0, 2 * sizeof(unsigned long long));
        if (!c->timing_ref) (void)hipEventCreate(&c->timing_ref);
        (void)hipDeviceSynchronize();
        (void)hipEventRecord(c->timing_ref, nullptr);
        (void)hipEventSynchronize(c->timing_ref);
    }
}

mpc_status mpc_kernel_timing_read(mpc_context* c, double* total_ms, long long* launches, double* busy_ms) {
    if (!c || !total_ms || !launches) return fail(MPC_ERR_ARGUMENT, "null argument");
    if (c->device < 0) return fail(MPC_ERR_NO_DEVICE, "context was created without a device");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    double sum = 0.0;
    std::vector<std::pair<float, float>> spans;
    for (size_t i = 0; i + 1 < c->timing_used; i += 2) {
        float a = 0.f, b = 0.f;
        HIP_TRY(hipEventElapsedTime(&a, c->timing_ref, c->timing_events[i]));
        HIP_TRY(hipEventElapsedTime(&b, c->timing_ref, c->timing_events[i + 1]));
        sum += b - a;
        spans.emplace_back(a, b);
    }
    // launches on the internal streams overlap: the union of their intervals is the time the machine spent in
    // this kernel
    std::sort(spans.begin(), spans.end());
    double busy = 0.0;
    float lo = 0.f, hi = -1.f;
    for (const auto& sp : spans) {
        if (hi < lo || sp.first > hi) {
            if (hi >= lo) busy += hi - lo;
            lo = sp.first;
            hi = sp.second;
        } else if (sp.second > hi) {
            hi = sp.second;
        }
    }
    if (hi >= lo) busy += hi - lo;
    *total_ms = sum;
    *launches = static_cast<long long>(c->timing_used / 2);
    if (busy_ms) *busy_ms = busy;
    c->timing_used = 0;
    return MPC_OK;
}

mpc_status mpc_kernel_counters_read(mpc_context* c, unsigned long long* mfma_instructions, unsigned long long* tile_channel_steps) {
    if (!c || !mfma_instructions || !tile_channel_steps) return fail(MPC_ERR_ARGUMENT, "null argument");
    if (c->device < 0) return fail(MPC_ERR_NO_DEVICE, "context was created without a device");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long v[2] = {0, 0};
    HIP_TRY(hipMemcpy(v, c->dd->stats, sizeof v, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(c->dd->stats, 0, sizeof v));
    *mfma_instructions = v[0];
    *tile_channel_steps = v[1];
    return MPC_OK;
}

mpc_status mpc_reserve(mpc_context* c, long long max_tiles) {
    if (!c || max_tiles < 1) return fail(MPC_ERR_ARGUMENT, "bad argument");
    if (c->device < 0) return fail(MPC_ERR_NO_DEVICE, "context was created without a device");
    HIP_TRY(hipSetDevice(c->device));
    return ensure_workspace(c, read_tuning(), max_tiles * 3);
}

mpc_status mpc_calc_mp(mpc_context* c, int channel, const double* quant_k, const double* input64,
                       mpc_basis_choice* choices, int* count) {
    if (!count) return fail(MPC_ERR_ARGUMENT, "null count");
    uint16_t n = 0;
    mpc_status st = mpc_calc_mp_batch(c, channel, quant_k, input64, 1, choices, &n, nullptr, nullptr);
    if (st == MPC_OK) *count = n;
    return st;
}

mpc_status mpc_quant_tables(int K, int block_size, double bpp_allocation, double* quant) {
    return guarded([&]() -> mpc_status {
    if (!quant) return fail(MPC_ERR_ARGUMENT, "null argument");
    if (K < 1 || K > MPC_MAX_K) return fail(MPC_ERR_ARGUMENT, "K=%d out of range 1..%d", K, MPC_MAX_K);
    if (block_size < 1 || block_size > 8) return fail(MPC_ERR_ARGUMENT, "block size %d out of range 1..8", block_size);
    if (!std::isfinite(bpp_allocation)) return fail(MPC_ERR_ARGUMENT, "bpp allocation must be finite");
    mpc::quantisation_tables(K, block_size, bpp_allocation, quant);
    return MPC_OK;
    });
}

int mpc_context_tile_encode_workgroups(const mpc_context* c) { return c ? c->user_workgroups.load() : 0; }

}  // extern "C"
