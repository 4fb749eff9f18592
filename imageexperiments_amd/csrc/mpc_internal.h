// mpc_internal.h -- product: what the translation units of libmpcodec.so share besides the public C ABI (include/mpcodec.h).
//   mpcodec_context.cpp    device dictionary, context, quantiser tables, pursuit launches, tile encode, timing, tuning switches
//   mpcodec_container.cpp  records on the device -> container (ContainerJob), the mpc_container_job_* API, the synchronous job (records_container)
//   mpcodec_pipeline.cpp   the frame pipeline (mpc_encode_image(s)*): frames -> tile encode -> container jobs, in stages
//   mpcodec_bitstream.cpp  host-only bitstream entry points
// and, behind host_bitstream.h (they know neither HIP nor the C ABI and also build on their own):
//   host_bitstream.cpp     bits, Golomb, Elias-Fano, Huffman, run lengths, the Huffman-or-Golomb choice, plan_stream, or_bits
//   host_container.cpp     the container: header, per-stream wrapper, the routes to a container, the parser
//   host_pool.cpp          the worker pool of the host stages
//   mpcodec_decode.cpp     tile reconstruction from records (mpc_decode_tiles_device), distortion, patch statistics
//   mpcodec_decode_seq.cpp the decoder of containers (mpc_decode_image, mpc_decode_images*), the device unpack of coded streams
//   mpcodec_index.cpp      the seek index's host-only entry points (mpc_container_index, mpc_parse_container_by_index)
//   mpcodec_debug.cpp      the tests' entry points to the screen's tables (mpc_debug_*, mpc_filter_tiles)
//   mpcodec_delta.cpp      the delta encoder (mpc_delta_*): diff against the kept frame, pursuit of the changed tiles only
//   mpcodec_patch.cpp      the delta stream's patches (mpc_patch_*): the format's entry points (host_patch.h) and the receiver session
//   mpcodec_budget.cpp     encode to a byte budget (mpc_encode_image_budget): depth profile, allocation, the search over the multiplier;
//                          encode to a target quality (mpc_encode_image_quality): the sweep over all multipliers, the pick, one allocation
//                          both for a group of frames (mpc_encode_images_budget, mpc_encode_images_quality): one multiplier for all frames
//   mpcodec_rate.cpp       a delta stream to a byte budget (mpc_delta_encode_patch_budget): the sent map, candidates, the search with floors
#pragma once

#include "../../include/mpcodec.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <vector>

#include "host_bitstream.h"
#include "host_dictionary.h"
#include "mp_device.h"

// the text mpc_last_error() returns on the calling thread (mpcodec_context.cpp)
extern "C" void mpc_set_error_text(const char* text);

struct mpc_context;
// what mpc_context_set_tile_encode_workgroups last set (0 = all CUs); mpc_rate_distortion restores it
extern "C" int mpc_context_tile_encode_workgroups(const mpc_context* ctx);

#pragma GCC visibility push(hidden)

// sets the calling thread's mpc_last_error() text, returns `st`
mpc_status fail(mpc_status st, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(call)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) return fail(MPC_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

inline mpc_status launch_failed(int err) {
    return fail(MPC_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(static_cast<hipError_t>(err)));
}

// what every entry point that needs the device answers a context made with device < 0
inline mpc_status no_device() { return fail(MPC_ERR_NO_DEVICE, "context was created without a device; there is no CPU fallback"); }

// No exception crosses the C ABI (the reference throws heap-allocated std::range_error*; here: status codes)
template <class F>
mpc_status guarded(F&& body) {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(MPC_ERR_ALLOC, "out of memory");
    } catch (const std::length_error& e) {
        return fail(MPC_ERR_ALLOC, "allocation size out of range: %s", e.what());
    } catch (const std::exception& e) {
        return fail(MPC_ERR_BITSTREAM, "%s", e.what());
    } catch (...) {
        return fail(MPC_ERR_BITSTREAM, "unknown failure");
    }
}

constexpr long long kMaxBatchDefault = 3LL * 524288;   // tile-channels in flight per call (an 8K frame in one go; ~1.5 GB of workspace)
constexpr unsigned kTripleCap = 1u << 20;              // (symbol, count, first position) triples the device entropy tables hold

// Environment switches of the library ("Environment switches").  None is needed in normal use and none changes a
// result; they exist for measurements and for tests that force rare paths.  read_tuning() reads them all, once per public
// entry call, on the calling thread; worker threads get what that thread read.
//   switch                        field            effect (default)
//   MPC_PATH=steps, MPC_FILTER=0  steps_path       the step-synchronous exhaustive f64 sweeps instead of the persistent kernel
//   MPC_PIPES                     pipes            concurrent sub-batches of those sweeps (by batch size, 1 - 4)
//   MPC_MAX_BATCH_TILES           max_batch        tiles in flight per sub-batch round of those sweeps (524288)
//   MPC_WORKGROUPS                workgroups       pursuit workgroups of every launch (all CUs)
//   MPC_SEQ_WORKGROUPS            seq_workgroups   pursuit workgroups of a frame sequence (7/8 of the CUs; 0 = all)
//   MPC_SEQ_GROUP                 seq_group        frames of a sequence that share one pursuit launch, 1 .. 3 (kSeqGroupDevice / kSeqGroupHost)
//   MPC_LAG_ASSEMBLY              lag_assembly     launch(g) waits for assembly + phase 1 of the frames of launch g - this (2)
//   MPC_LAG_PHASE2                lag_phase2       ... and for phase 2 of the frames of launch g - this (3)
//   MPC_SINGLE_STRIPES            single_stripes   row stripes of a single host frame (1 below 32 MB, 3, 4 from 80 MB)
//   MPC_HOST_ENTROPY=1            host_entropy     the entropy stage on the host
//   MPC_ENTROPY_TRIPLES           triple_limit     distinct symbols per frame above which a frame takes the host route (2^20)
//   MPC_TRACE=1                   trace            per-frame time stamps of the pipeline and the decoder on stderr
// MPC_HOST_THREADS (worker threads of the host's table building and parsing) is read by host_pool.cpp (host_thread_count).
// frames per pursuit launch of a sequence.  Device frames at 4928x3264: 1 / 2 / 3 -> 5 287 / 5 347 / 4 597 Mpix/s
// (three per launch leave the six slots two groups); host frames -> bytes: 4 879 / 4 826 Mpix/s with 1 / 2 (a launch waits for all
// its uploads)
constexpr int kSeqGroupDevice = 2;
constexpr int kSeqGroupHost = 1;
struct Tuning {
    bool steps_path = false, host_entropy = false, trace = false;
    int pipes = 0, workgroups = 0, single_stripes = 0;          // > 0: forced
    int seq_workgroups = -1;                                    // >= 0: forced
    int lag_assembly = 2, lag_phase2 = 3;
    int seq_group = 0;                                          // > 0: forced
    long long max_batch = kMaxBatchDefault;
    unsigned triple_limit = kTripleCap;
};
Tuning read_tuning();

double trace_ms();                      // milliseconds since the first call (MPC_TRACE)

// mpc_container_index_device with the scan's sizes given (0 = the defaults): what it and mpc_debug_container_index_device call
mpc_status container_index_on_device(mpc_context* c, const uint8_t* bytes, size_t nbytes, int interval, unsigned flags, int segment_bits,
                                     int window_bits, uint8_t** index, size_t* index_bytes, int* route);

// A grow-only device, pinned or mapped pinned buffer.  Growing frees the old buffer after a device synchronisation (the device
// may still read it): free in steady state, where nothing grows.
struct GrowBuffer {
    enum Kind { kDevice, kPinned, kMapped };
    Kind kind;
    void* p = nullptr;
    size_t bytes = 0;
    explicit GrowBuffer(Kind k) : kind(k) {}
    GrowBuffer(const GrowBuffer&) = delete;
    GrowBuffer& operator=(const GrowBuffer&) = delete;
    ~GrowBuffer() { release(); }
    // at least `need` bytes; *grown (optional): the buffer is a new one
    mpc_status reserve(size_t need, const char* what, bool* grown = nullptr);
    void release();
    char* data() const { return static_cast<char*>(p); }
};

// a device allocation for the length of one call
struct DeviceTemp {
    void* p = nullptr;
    ~DeviceTemp() { (void)hipFree(p); }
};

// Hands out 256-byte aligned pieces of one allocation in order; on a null base it only adds up their sizes.
struct Carve {
    char* base = nullptr;
    size_t at = 0;
    static size_t up(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }
    template <class T>
    T* take(size_t count) {
        T* p = base ? reinterpret_cast<T*>(base + at) : nullptr;
        at += up(sizeof(T) * count);
        return p;
    }
};

// The stream assembly's buffers in a slot, after the records: block_live | sizes, and for the assembly (not the decoder's gather)
// | stream offsets | symbols (worst case: every record alive) | dc.  Fills the StreamArgs pointers.
void carve_stream_buffers(Carve& cv, long long tiles, int K, bool assembly, mpc::StreamArgs* sa);

// [lo, hi) of a host frame to `dst` on `stream` through `pinned` (same offsets), in at least 1 MiB chunks, about `parts` of them, on
// a few threads: a chunk goes to the device as soon as it is in pinned memory (the caller's memory is pageable: the runtime would
// stage it through one thread at a few GB/s)
hipError_t staged_upload(int device, const uint8_t* src, uint8_t* pinned, uint8_t* dst, size_t lo, size_t hi, size_t parts,
                         hipStream_t stream);

#pragma GCC visibility pop

// Everything on the device that depends only on (device, block size): the dictionary in double, its filter copies, the
// Gram table and the persistent kernel's scratch, streams and queues.  Shared by every context of the process on that
// device (a context adds K and the quantisation tables): the Gram table alone is 12.6 GB.  All persistent-kernel launches
// of the process go through the three per-channel streams held here, which also serialises their use of the scratch.
struct DeviceDict {
    int device = -1;
    int base_rows_padded = 0, num_base = 0, num_cus = 0;
    long long detail_rows = 0;
    double* d_base = nullptr;
    double* d_detail = nullptr;
    float* d_base32 = nullptr;        // the same rows rounded to float (the `...Fast` flavour), same layout
    float* d_detail32 = nullptr;
    int32_t* d_rows = nullptr;
    int32_t* d_rowoff = nullptr;
    uint16_t* d_base_t1 = nullptr;    // split-bf16 filter copies in MFMA operand order (persistent kernel)
    uint16_t* d_detail_t1 = nullptr;
    uint8_t* d_shadow = nullptr;      // [3][detail_rows]
    float* d_gram = nullptr;          // [3][num_base + detail_rows][num_base * 64]
    std::mutex launch_lock;           // one enqueue sequence at a time
    hipEvent_t done[1] = {};          // recorded behind every launch: the next one (any stream) waits for it
    int workgroups = 0;               // scratch is sized for this many workgroups per launch
    float* pair_p = nullptr;          // per-wave scratch of the persistent kernel (pairs: approximations, meta, bounds)
    unsigned* pair_meta = nullptr;
    float* pair_e = nullptr;
    unsigned* queues = nullptr;       // [3]
    unsigned long long* stats = nullptr;   // [2]: MFMA instructions, tile-channel-steps executed by the persistent kernel since the last reset
    ~DeviceDict() {
        if (device < 0) return;
        (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();
        (void)hipFree(d_base); (void)hipFree(d_rows); (void)hipFree(d_rowoff);      // d_detail / d_detail32: inside d_base / d_base32
        (void)hipFree(d_base32);
        (void)hipFree(d_base_t1); (void)hipFree(d_detail_t1);
        (void)hipFree(d_shadow); (void)hipFree(d_gram); (void)hipFree(queues); (void)hipFree(stats);
        (void)hipFree(pair_p); (void)hipFree(pair_meta); (void)hipFree(pair_e);
        if (done[0]) (void)hipEventDestroy(done[0]);
    }
};

#pragma GCC visibility push(hidden)

// ---- device entropy stage (mpcodec_container.cpp) ----
// a slot's grow-only buffers; `tiles`, `K`: the geometry the tables inside `dev` were last cleared for
struct EntropySlot {
    GrowBuffer dev{GrowBuffer::kDevice};
    GrowBuffer host{GrowBuffer::kMapped};
    size_t tiles = 0;
    int K = 0;
};

struct EntropyBuffers {
    mpc::EntropyArgs args{};
    uint8_t* d_out = nullptr;
    size_t out_capacity = 0;             // bytes, device and host
    unsigned long long capacity_symbols = 0;
    // pinned
    mpc::EntStream* h_streams = nullptr;
    unsigned* h_totals = nullptr;
    unsigned* h_triples = nullptr;
    unsigned* h_entries = nullptr;
    uint8_t* h_out = nullptr;
    // the seek index's checkpoints (with_index only): args.checkpoints on the device, their pinned copy
    unsigned long long* h_checkpoints = nullptr;
    // index version 2's aux entries (with_index == 2 only): args.aux on the device, their pinned copy
    unsigned long long* h_aux = nullptr;
};

// carve (and grow) a slot's entropy buffers for frames of `tiles` tiles; the symbols of the streams live in the caller's buffers.
// with_index: the checkpoint arrays as well, behind everything else -- a slot never used with an index holds none, and one that
// was keeps them (grow-only) without moving anything when a call comes without.  with_index == 2: behind those, in the same way, what
// index version 2 needs (the aux entries, their offsets per stream, the step-0 streams' sums per block)
mpc_status entropy_buffers(EntropySlot& e, size_t tiles, int K, EntropyBuffers* b, int with_index = 0);

// What the host keeps of a frame between the tables step and the collect step of the device route.
struct EntropyPending {
    std::vector<mpc::StreamPlan> plans;
    mpc::BitWriter head;
    size_t total_bytes = 0;
    size_t n_aux = 0;                    // index version 2: aux entries on their way to the host
};

// Records on the device -> container bytes: the only code that does this (the frame pipeline, mpc_container_job_*,
// mpc_code_symbol_streams_device).  The caller sets the first block of fields, then runs the steps in order:
//   container_begin    stream assembly (unless the symbols are given) and entropy phase 1 on `side`, then `phase1`
//   container_tables   waits for `phase1`, builds the code tables, enqueues phase 2 and the container's copy on `down`, then
//                      `done`; `enqueued` (optional) is called once that is on the stream or clear that it will not be.  The
//                      host route (MPC_HOST_ENTROPY, or a frame the device tables cannot hold) makes the container here instead.
//   container_collect  waits for `done`, patches the head and the streams' pre and post bits in
// With index_interval set the job also leaves the container's seek index in `index`, the blob mpc_container_index would build
// from the finished container: on the device route from the plans and the checkpoints the code kernel recorded (index_from_plan;
// the pinned copy of the checkpoints travels on `down` behind the container's, in front of `done`), on the host route by
// build_container_index.  With index_expanded as well the index is version 2: phase 1 leaves the aux entries on the device, their
// pinned copy travels with the checkpoints', and index_from_plan checks them against the plans; entries it refuses, and the host
// route, get the blob from build_container_index(..., expanded) of the finished container.
struct ContainerJob {
    hipStream_t side = nullptr, down = nullptr;
    hipEvent_t phase1 = nullptr, done = nullptr;
    bool spin = false;                   // poll the events (a single frame) instead of sleeping on them
    GrowBuffer* host_stage = nullptr;    // the host route downloads counts, offsets and symbols to here, from `host_offset` on ...
    size_t host_offset = 0;
    const uint16_t* h_counts = nullptr;  // ... unless they are on the host already
    const unsigned long long* h_stream_off = nullptr;
    const uint16_t* h_symbols = nullptr;
    unsigned index_interval = 0;         // 0 = no index, else 32 ... 65536; needs `eb` carved with_index
    bool index_expanded = false;         // index version 2 (MPC_INDEX_EXPANDED); needs `eb` carved with_index == 2
    // set by container_begin
    int width = 0, height = 0, K = 0, block_size = 0;
    std::vector<double> quant;
    mpc::StreamArgs sa{};
    bool device_entropy = false;         // false: the host route
    EntropyBuffers eb{};
    unsigned triple_limit = kTripleCap;
    EntropyPending pending;
    uint8_t* blob = nullptr;             // the host route's container
    size_t nblob = 0;
    std::vector<uint8_t> index;          // the result with index_interval set, complete after container_collect
    double stamps[5] = {};               // MPC_TRACE: phase 1 done, statistics read, tables built, symbols on the host, bytes on the host
    ~ContainerJob() { std::free(blob); }
};

// `buffers`: where the stream assembly's are carved (carve_stream_buffers), or null when d_symbols / d_stream_off hold the
// streams already; `eb`: the entropy slot's buffers (entropy_buffers), null for the host route
mpc_status container_begin(ContainerJob& j, const mpc_context* c, const EntropyBuffers* eb, unsigned triple_limit, char* buffers,
                           const uint16_t* d_counts, const uint32_t* d_choices, uint16_t* d_symbols,
                           unsigned long long* d_stream_off, int width, int height, const double* quant);
mpc_status container_tables(ContainerJob& j, const std::function<void()>& enqueued = nullptr);
mpc_status container_collect(ContainerJob& j, uint8_t** bytes, size_t* nbytes);

// the host route's pinned buffers: counts | stream offsets | symbols (worst case: every record alive); on a null base only their size
struct HostRoute {
    uint16_t* counts;
    unsigned long long* stream_off;
    uint16_t* symbols;
};
size_t host_route_layout(char* base, size_t n_tc, int K, HostRoute* r);

// the `interval` and `flags` arguments of the indexed entry points (mpcodec_container.cpp)
mpc_status index_interval_of(int interval, unsigned* out);
mpc_status index_flags_of(unsigned flags, bool* expanded);
// the `index_interval` argument of the entry points whose index is optional: below 0 = none (*every = 0), else as index_interval_of
inline mpc_status optional_index_interval_of(int interval, unsigned* every) {
    if (interval >= 0) return index_interval_of(interval, every);
    *every = 0;
    return MPC_OK;
}

// A slot of the mpc_container_job_* API.  Its buffers are its own: the context's entropy slots and staging belong to the frame
// pipeline (mpc_encode_image(s)) and to mpc_code_symbol_streams_device, which may run -- and re-carve or clear their tables --
// between `begin` and `collect`.
struct JobSlot {
    int stage = 0;                       // 0 idle, 1 begun, 2 tables done
    ContainerJob job;
    EntropySlot ent;
    GrowBuffer dev{GrowBuffer::kDevice}; // stream assembly buffers
    ~JobSlot() {
        if (job.phase1) (void)hipEventDestroy(job.phase1);
        if (job.done) (void)hipEventDestroy(job.done);
    }
};

#pragma GCC visibility pop

#pragma GCC visibility push(hidden)
// A frame in flight in the decoder (mpc_decode_image, mpc_decode_images*; a call of one frame uses slot 0): its own stream, buffers, error words and event, so that frames overlap and a call
// waits for nothing but its own work.
struct DecodeSlot {
    GrowBuffer pinned{GrowBuffer::kPinned};   // the error words; the coded streams on their way in, later the pixels on their way out
    GrowBuffer dev{GrowBuffer::kDevice};
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    hipEvent_t stamp[7] = {};                 // MPC_TRACE: before the upload, the unpack, the gather, the pixels' copy, after it;
                                              // [5]: behind the device parse (a frame with a seek index), in front of the unpack;
                                              // [6]: a window of a frame: behind the lengths stream's parse and the ranks
    ~DecodeSlot() {
        if (stream) (void)hipStreamDestroy(stream);
        if (done) (void)hipEventDestroy(done);
        for (hipEvent_t e : stamp)
            if (e) (void)hipEventDestroy(e);
    }
};
#pragma GCC visibility pop

struct mpc_context {
    int K = 0, block_size = 0, device = -1;
    double bpp = 0.0;
    bool fast = false;                // the `...Fast` (float) flavour of the tile path (mpc_context_set_fast)
    mpc::Dictionary dict;
    std::vector<double> quant;        // [3*K]
    std::shared_ptr<DeviceDict> dd;   // owns the dictionary's device residents
    double* d_quant = nullptr;        // the context's tables; only mpc_context_set_quant changes them
    // per-call quantiser overrides (the `quant` argument of the encode / decode entry points) go to a ring of device
    // slots of their own, so that a later call with quant == NULL still quantises with the context's tables
    static constexpr int kQuantSlots = 16;
    double* d_quant_ring = nullptr;   // [kQuantSlots][3 * MPC_MAX_K]
    hipEvent_t quant_free[kQuantSlots] = {};         // behind the last reader of each slot (CallQuant)
    unsigned quant_next = 0;
    std::mutex quant_lock;            // one call with an override at a time per context, from taking its slot to recording quant_free
    std::recursive_mutex host_calls;  // the host-buffer entry points share the staging buffers below
    int* d_flag = nullptr;            // mpc_decode_tiles_device: set when a record indexes outside its dictionary
    int* d_crop_flag = nullptr;       // mpc_crop_records_device: set by a count above K, read by mpc_crop_records_check
    GrowBuffer delta_scratch{GrowBuffer::kDevice};   // mpc_tile_diff_device: the flags and block counts (mpc::tile_diff_scratch_bytes)
    GrowBuffer compose_dev{GrowBuffer::kDevice};     // mpc_compose_indexed: the destination's records, the owner map, the pixel parts' patches
    hipStream_t compose_side = nullptr;              // ... the pixel parts' stream and the final container job's, made on first use
    GrowBuffer budget_dev{GrowBuffer::kDevice};      // mpc_encode_image_budget: the frame, its records, the cut counts, the profile, two depth maps
    hipStream_t budget_stream = nullptr;             // ... everything of such a call, made on first use
    // grow-only staging for the host-buffer encode entry points (mpc_encode_tiles / mpc_encode_image(s)): allocating and freeing
    // them per call cost several times the encode itself.  The decoder stages in its slots' own buffers (DecodeSlot).
    GrowBuffer stage{GrowBuffer::kDevice};
    GrowBuffer host_stage{GrowBuffer::kPinned};
    // mpc_encode_images: upload / compute / download streams and per-slot events (upload done, pursuit done, download done)
    hipStream_t seq_up = nullptr, seq_compute = nullptr;
    // read by device-pointer encodes, which do not take `host_calls`: a stale value costs or gains a few workgroups, nothing else
    std::atomic<int> seq_workgroups{0};              // > 0: the pursuits of a frame sequence leave CUs to the kernels behind them
    std::atomic<int> user_workgroups{0};             // > 0: mpc_context_set_tile_encode_workgroups
    static constexpr int kSeqSlots = 6;              // frames in flight in mpc_encode_images (a frame's container is ready about
                                                     // three pursuits after its own started)
    hipEvent_t seq_events[kSeqSlots][3] = {};
    static constexpr int kSingleStripes = 4;
    hipEvent_t seq_stripe_up[kSingleStripes] = {};   // a single host frame goes up and is encoded in row stripes (encode_sequence)
    hipEvent_t seq_pursuit_done[kSeqSlots] = {};      // behind a slot's pursuit, for the slot's own stream to wait on
    // the side streams of all slots: [0] stream assembly + phase 1, [1] phase 2 and the copies.  The others are created and never
    // used: without them a single 16 Mpixel host frame takes 2 % longer and a single 1080p frame 6 % less
    // (profiles/pipeline_stages.txt; measured, not explained -- a choice by frame size would be a change of speed of its own)
    hipStream_t seq_down[kSeqSlots] = {};
    // device-side entropy stage (mp_entropy.hip): per-slot buffers of the frame pipeline and mpc_code_symbol_streams_device
    EntropySlot ent[kSeqSlots];
    std::unique_ptr<JobSlot> jobs[kSeqSlots];        // mpc_container_job_*: records on the device -> container, in steps
    static constexpr int kDecodeSlots = 6;           // frames in flight on the device in a decode call
    std::unique_ptr<DecodeSlot> dec[kDecodeSlots];   // created on first use
    // The exhaustive path's pursuit of a call is cut into sub-batches that run on `pipes` internal streams, each with its own
    // workspace: the latency-bound bookkeeping kernels of one sub-batch (finish, update, bucket, fill) overlap the
    // machine-filling sweeps of the other.  Fork/join with events on the caller's stream: still no host synchronisation.
    struct Pipe {
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;
        void* mem = nullptr;
        mpc::Workspace ws{};
    };
    std::vector<Pipe> pipes;
    hipEvent_t fork = nullptr;
    int ws_cap = 0;                   // tile-channels per pipe workspace
    int max_waves = 0;
    int num_cus = 0;
    // optional live timing of the base-sweep launches (mpc_kernel_timing_*)
    bool timing = false;
    std::vector<hipEvent_t> timing_events;      // 2 per launch, grown on demand
    size_t timing_used = 0;
    hipEvent_t timing_ref = nullptr;            // common time origin for the union of launch intervals
};

#pragma GCC visibility push(hidden)

// ---- decode (mpcodec_decode.cpp) ----
// FromCoeffsDynamic + RGBFromYUV for whole tiles on `stream`; d_quant: [3][K] doubles on the device; d_flag: the caller's error
// word (zeroed on `stream` first, set when a record indexes outside its dictionary)
mpc_status decode_tiles_on_device(mpc_context* c, const uint16_t* d_counts, const uint32_t* d_choices, const double* d_quant, int K,
                                  int width, int height, uint8_t* d_rgb, int* d_flag, void* stream, const mpc::DecodeWindow* window = nullptr,
                                  const mpc::DecodeView* view = nullptr);

// ---- views (include/mpcodec.h, "views"): what the entry points of mpcodec_index.cpp and mpcodec_decode_seq.cpp share ----
// a view's own arguments: nullptr, or what is wrong with them
inline const char* view_argument_error(const mpc_view& v) {
    if (v.steps < 0) return "steps must not be negative";
    if (v.scale_log2 < 0 || v.scale_log2 > 3) return "scale_log2 must be 0 ... 3";
    const int c = 1 << v.scale_log2;
    if (v.rect.x % c != 0 || v.rect.y % c != 0) return "the rectangle's origin must be a multiple of the reduction";
    return nullptr;
}
// the rectangle a view names in a frame of width x height: (0, 0, 0, 0) is the whole frame
inline mpc_rect view_rect(const mpc_view& v, int width, int height) {
    const mpc_rect& r = v.rect;
    return r.x == 0 && r.y == 0 && r.width == 0 && r.height == 0 ? mpc_rect{0, 0, width, height} : r;
}
// pixels of `extent` reduced by 2^scale_log2
inline int view_extent(int extent, int scale_log2) { return (extent + (1 << scale_log2) - 1) >> scale_log2; }
// the steps a view keeps of a container of K: 0 = all, above K acts as K
inline int view_steps(int steps, int K) { return steps > 0 && steps < K ? steps : K; }

// a transcode's view (include/mpcodec.h, "transcode"): nullptr, or what is wrong with the arguments that need no container
inline const char* transcode_argument_error(const mpc_view& v) {
    if (v.steps < 0) return "steps must not be negative";
    if (v.scale_log2 != 0) return "scale_log2 must be 0: a transcode does not reduce";
    return nullptr;
}

// a compose's parts (include/mpcodec.h, "compose") as the host's plan takes them
inline std::vector<mpc::ComposePart> compose_parts(const mpc_part* parts, int n_parts) {
    std::vector<mpc::ComposePart> made(static_cast<size_t>(n_parts > 0 ? n_parts : 1));      // never empty: data() is no null pointer
    for (size_t p = 0; n_parts > 0 && p < made.size(); ++p) {
        made[p].source = parts[p].source;
        made[p].x = parts[p].rect.x;
        made[p].y = parts[p].rect.y;
        made[p].w = parts[p].rect.width;
        made[p].h = parts[p].rect.height;
        made[p].dx = parts[p].x;
        made[p].dy = parts[p].y;
        made[p].has_pixels = parts[p].rgb != nullptr;
    }
    return made;
}

// the context's crop error word, made on first use; the device is current (mpcodec_container.cpp)
extern "C" mpc_status crop_flag(mpc_context* c);

// ---- context and tile encode (mpcodec_context.cpp) ----
mpc::DictDevice dict_device(const mpc_context* c);
// The device table a call quantises with: the context's, or a ring slot holding the call's override.  The override is written on
// `s` by a kernel that carries it as an argument (`quant` is read before call_quant returns; nothing waits for the stream).  A slot
// is handed out again only behind the event its last user recorded when it let go of it, so the streams of a context's calls need
// not be one: the call keeps its CallQuant alive until everything that reads d_q is enqueued on `s`.  Calls with an override from
// several host threads take turns (quant_lock, held from the slot's hand-out to that record), so the event a slot's next user waits
// on has always been recorded.
struct CallQuant {
    const double* d_q = nullptr;
    CallQuant() = default;
    CallQuant(const CallQuant&) = delete;
    CallQuant& operator=(const CallQuant&) = delete;
    ~CallQuant();
    mpc_context* ctx = nullptr;
    int slot = -1;                    // -1: the context's own table, nothing to let go of
    hipStream_t stream = nullptr;
    std::unique_lock<std::mutex> hold;               // mpc_context::quant_lock, while the call has an override
};
mpc_status call_quant(mpc_context* c, const double* quant, hipStream_t s, CallQuant* q);
// the same with the quantiser steps the container header carries (mpc::header_quant of `quant`, or of the context's tables)
mpc_status header_quant_device(mpc_context* c, const double* quant, hipStream_t s, CallQuant* cq);
// MPC_ERR_ARGUMENT if `stream` is being captured into a graph (nothing has been enqueued then): the entry points that take a
// stream use per-context and per-process scratch whose order a replayed graph would not take part in
mpc_status refuse_capture(void* stream);
mpc_status ensure_workspace(mpc_context* c, const Tuning& t, long long tile_channels);
// whole_frame_order: the records go where one launch over the whole frame would put them (FrameInput::out_tile_rows) and the
// caller has zeroed d_choices for the whole frame (stripes of one frame encoded one by one, encode_sequence's single frames)
// table: the frames of the launch lie anywhere and so do their records in d_counts / d_choices (mpc::FrameTable)
mpc_status encode_batch_device(mpc_context* c, const Tuning& t, const uint8_t* d_rgb, int frames, size_t frame_stride, int width,
                               int height, size_t row_stride, int tile_row_begin, int tile_row_end, const double* quant,
                               uint16_t* d_counts, mpc_basis_choice* d_choices, double* d_energy, uint32_t* d_swept, void* stream,
                               bool whole_frame_order, const mpc::FrameTable* table = nullptr);

// ---- records -> container for a synchronous caller (mpcodec_container.cpp): the delta encoder, the cut encodes and the rate search ----
// a container and its seek index in malloc'ed memory, released unless taken
struct ContainerMade {
    uint8_t* bytes = nullptr;
    size_t nbytes = 0;
    std::vector<uint8_t> index;
    ContainerMade() = default;
    ContainerMade(const ContainerMade&) = delete;
    ContainerMade& operator=(const ContainerMade&) = delete;
    ~ContainerMade() { std::free(bytes); }
    void swap(ContainerMade& o) {
        std::swap(bytes, o.bytes);
        std::swap(nbytes, o.nbytes);
        index.swap(o.index);
    }
};
// One records-to-container job on job slot 0 with everything on `s`, as a compose finishes: the container of `d_counts` / `d_choices`
// (the caller's records and geometry), and with `every` != 0 its seek index from the entropy stage: version 2, or with `expanded`
// false version 1 (what a patch carries).  The call waits for the container; the slot is left as mpc_container_job_begin expects it
mpc_status records_container(mpc_context* c, const Tuning& tuning, hipStream_t s, const uint16_t* d_counts, const mpc_basis_choice* d_choices,
                             long long tiles, int width, int height, const double* quant, unsigned every, ContainerMade* out,
                             bool expanded = true);
// `made` to the caller of an entry point: the container, and with `every` != 0 a malloc'ed copy of its seek index
mpc_status deliver_container(ContainerMade& made, unsigned every, uint8_t** bytes, size_t* nbytes, uint8_t** index, size_t* index_bytes);

// ---- rate control on the device (mpcodec_budget.cpp): the depth profile of records against the tight frame they came from ----
mpc_status profile_on_device(mpc_context* c, const uint16_t* d_counts, const mpc_basis_choice* d_choices, const double* quant,
                             const uint8_t* d_rgb, int width, int height, uint32_t* d_profile, int* d_error, hipStream_t s);
// The search over the multiplier table (host_budget.h) of the budget encode and of the delta stream's budget call: the smallest
// multiplier whose result fits.  probe(j, &fits) makes the result at j and keeps it where it fits.  The last multiplier, the smallest
// result there is, goes first, with `behind_first` once behind it (the error word of the kernels that ran in front of its end); then
// the bisection between the full result, which does not fit, and that one.  *found: the multiplier, or -1 where not even the last one
// fits, which the caller refuses in its own words
mpc_status multiplier_search(const std::function<mpc_status(int, bool*)>& probe, const std::function<mpc_status()>& behind_first, int* found);

#pragma GCC visibility pop
