// mpcodec_pipeline.cpp -- product: the frame pipeline behind mpc_encode_image(s)[_indexed[2]][_device], compressed::encodeImage
// for a sequence of equally sized frames: device tile encode, then records -> container (ContainerJob, mpcodec_container.cpp)
// -- pipelined over kSeqSlots slots.  Frames come from host memory (uploaded through the slot's pinned image on an upload
// stream) or are already resident on the device.  index_interval != 0: every frame's seek index as well (indexes, index_bytes),
// version 2 if index_expanded.
//
// The pipeline's streams.  `seq_compute`: the pursuits, one behind the other.  Side stream A: behind pursuit(f) (an event) the
// stream assembly and entropy phase 1 of frame f.  Side stream B: phase 2 and the container's copy of frame f, enqueued by the
// frame's worker once it has built the code tables from phase 1's statistics (mapped host memory written by the kernels
// themselves; the host waits on events only).  A pursuit launch covers a group of frames (below); launch L waits (events) for
// the assembly + phase 1 of the frames of launch L - 2 and for the phase 2 of those of launch L - 3, so nothing piles up; with
// the CUs the pursuits leave free (below) both chains run beside the pursuits of the following frames.  The shapes this
// replaced -- everything on one ordered queue; phase 2 alone on a side stream -- are in DESIGN.md 4 and 9.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <future>
#include <utility>

#include "mpc_internal.h"

namespace {
constexpr int S = mpc_context::kSeqSlots;

// One call's pipeline: encode_sequence (below) fills in the call and runs the stages.
struct FramePipeline {
    mpc_context* const c;
    const Tuning t;
    const uint8_t* const* const frames;
    const bool on_device;
    const int n_frames, width, height;
    const double* const quant;
    uint8_t** const bytes;
    size_t* const nbytes;
    const unsigned index_interval;
    uint8_t** const indexes;
    size_t* const index_bytes;
    const bool index_expanded;
    // geometry
    const int K = c->K, tiles_y = (height + 7) / 8;
    const size_t tiles = static_cast<size_t>((width + 7) / 8) * tiles_y, n_tc = tiles * 3, img_bytes = static_cast<size_t>(3) * width * height;
    // device slot: [image] | stream assembly;  host slot: [image] | the host route's counts, offsets, symbols.  The slots' counts
    // and records lie in front of the device slots as two arrays [slot][record]: a launch over a group of frames addresses
    // every frame's records by one record index (mpc::FrameTable)
    size_t streams_at = 0, dev_slot = 0, route_at = 0, host_slot = 0;      // `dev`, `host`: offsets in a slot, a slot's size
    size_t counts_at = 0, choices_at = 0, slots_at = 0;                   // `records`: offsets in the device staging
    const int n_slots = std::min(S, n_frames);
    // a single frame: nothing to overlap with, so its worker runs on the calling thread (no thread to start and to join) and
    // polls the device instead of sleeping
    const bool single = n_frames == 1;
    int single_stripes = 1, G = 1;
    bool striped_single = false;
    hipStream_t pursuit_stream = nullptr;
    struct Pending {
        std::future<std::pair<uint8_t*, size_t>> result;     // malloc'ed container, or {nullptr, 0}
        int frame = -1;
    };
    std::future<void> phase2_enqueued[S];
    EntropyBuffers ent[S];
    ContainerJob jobs[S];
    Pending pending[S];
    std::future<hipError_t> uploads[S];
    mpc_status st = MPC_OK;

    ~FramePipeline() { c->seq_workgroups = 0; }                           // the pursuits' workgroup limit holds for the call (prepare)

    char* dev_slot_base(size_t sl) const { return c->stage.data() + slots_at + sl * dev_slot; }
    char* host_slot_base(size_t sl) const { return c->host_stage.data() + sl * host_slot; }
    // a slot's counts and records; slot 0's are the whole arrays
    uint16_t* slot_counts(size_t sl) const { return reinterpret_cast<uint16_t*>(c->stage.data() + counts_at) + sl * n_tc; }
    mpc_basis_choice* slot_choices(size_t sl) const { return reinterpret_cast<mpc_basis_choice*>(c->stage.data() + choices_at) + sl * n_tc * K; }

    // The pipeline's streams and events, on a context's first sequence.  The side streams at the highest priority, the pursuits'
    // at the lowest: CUs a pursuit gives up at its end go to the waiting chains of small kernels before the next pursuit's
    // workgroups.  Two side streams for all slots: the runtime maps streams onto a handful of hardware queues, and a slot stream
    // that lands on the pursuit stream's queue lines its kernels up behind the next pursuit -- with three streams in all nothing
    // has to share.  seq_down[0], side A: stream assembly + phase 1; seq_down[1]: phase 2, the container's copy, the host
    // route's copies; the context's other side streams are made and left idle (mpc_context::seq_down).  Equal priorities and
    // one side stream per slot were measured and dropped: DESIGN.md 9, profiles/pipeline_switches.txt.
    mpc_status make_streams() {
        if (c->seq_up) return MPC_OK;
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        const bool prio = least != greatest;
        HIP_TRY(hipStreamCreateWithFlags(&c->seq_up, hipStreamNonBlocking));
        HIP_TRY(prio ? hipStreamCreateWithPriority(&c->seq_compute, hipStreamNonBlocking, least) : hipStreamCreateWithFlags(&c->seq_compute, hipStreamNonBlocking));
        for (auto& s : c->seq_down)
            HIP_TRY(prio ? hipStreamCreateWithPriority(&s, hipStreamNonBlocking, greatest) : hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        for (hipEvent_t& e : c->seq_pursuit_done) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (hipEvent_t& e : c->seq_stripe_up) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        // blocking events: a thread waiting for the device sleeps instead of spinning (the entropy stage wants the cores)
        for (auto& slot : c->seq_events)
            for (hipEvent_t& e : slot) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventBlockingSync));
        return MPC_OK;
    }

    mpc_status prepare() {
        Carve dev, host;
        (void)dev.take<uint8_t>(on_device ? 0 : img_bytes);
        (void)host.take<uint8_t>(on_device ? 0 : img_bytes);
        streams_at = dev.at;
        mpc::StreamArgs measured{};
        carve_stream_buffers(dev, static_cast<long long>(tiles), K, true, &measured);
        HostRoute unused;
        route_at = host.at;
        dev_slot = dev.at;
        host_slot = route_at + host_route_layout(nullptr, n_tc, K, &unused);
        // a sequence gets every slot's buffers at once: a later, longer call then finds them (allocating pinned memory takes
        // tens of milliseconds)
        const size_t alloc_slots = n_frames > 1 ? S : 1;
        Carve records;
        counts_at = records.at;
        (void)records.take<uint16_t>(alloc_slots * n_tc);
        choices_at = records.at;
        (void)records.take<mpc_basis_choice>(alloc_slots * n_tc * K);
        slots_at = records.at;
        if (const mpc_status gs = c->host_stage.reserve(alloc_slots * host_slot, "pinned staging"); gs != MPC_OK) return gs;
        if (const mpc_status gs = c->stage.reserve(slots_at + alloc_slots * dev_slot, "device staging"); gs != MPC_OK) return gs;
        if (const mpc_status ss = make_streams(); ss != MPC_OK) return ss;
        pursuit_stream = c->seq_compute;
        if (const mpc_status ws = ensure_workspace(c, t, static_cast<long long>(n_tc)); ws != MPC_OK) return ws;
        // A pursuit on every CU leaves the small kernels behind the previous frames' pursuits (stream assembly, entropy phases: ~8 %
        // of a frame's CU time) nowhere to run but the gap between two pursuits, where they are latency-bound and the chip idles for
        // ~0.45 ms per 16 Mpixel frame.  With one CU in eight left free they run beside the pursuit instead.  Measured on one box
        // (tools/ab_env_bench.sh, MPC_SEQ_WORKGROUPS = pursuit workgroups of 256): 4928x3264 K=32  256: 4 780, 240: 4 620, 224: 5 060,
        // 216: 4 980, 208: 4 870 Mpix/s; 1920x1080 K=8  256: 3 300 - 3 790, 224: 4 150; 7680x4320 K=16  256: 5 570, 224: 5 860 (with
        // 16 CUs the chains cannot keep up and the pursuits wait for them).
        if (!single && c->num_cus >= 16) c->seq_workgroups = t.seq_workgroups >= 0 ? t.seq_workgroups : c->num_cus - c->num_cus / 8;
        if (!t.host_entropy)
            for (size_t sl = 0; sl < alloc_slots; ++sl)
                if (const mpc_status es = entropy_buffers(c->ent[sl], tiles, K, &ent[sl], index_interval ? (index_expanded ? 2 : 1) : 0);
                    es != MPC_OK)
                    return es;
        // a single host frame in row stripes (launch_striped); needs the persistent kernel (the step-synchronous cross-check path
        // writes stripe order only).  Measured (tools/single_frame_trace.py, host RGB -> bytes): 4928x3264  1 / 2 / 3 / 4 stripes:
        // 5.69 / 5.25 / 4.92 / 5.20 ms; 1920x1080: 1.24 / 1.42 / 1.45 / 1.63 ms -- every further launch costs a prologue (144 KiB of
        // LDS per workgroup) and a tail, more than a 6 MB copy takes; 7680x4320: 9.5 / 8.3 / 8.1 ms with 1 / 3 / 4
        single_stripes = t.single_stripes > 0 ? t.single_stripes
                                              : (img_bytes >= (size_t(80) << 20) ? 4 : (img_bytes >= (size_t(32) << 20) ? 3 : 1));
        striped_single = single && !on_device && single_stripes > 1 && tiles_y >= 4 * single_stripes && !t.steps_path;
        // Frames f .. f + gn - 1 share one pursuit launch (MPC_SEQ_GROUP): the kernel runs them as one batch -- one queue per channel
        // over all of them -- so the prologue (144 KiB of LDS per workgroup), the tail in which the CUs run dry and the gap between two
        // launches are paid once per group.  Everything behind the launch stays per frame.  A single frame and the step-synchronous
        // cross-check path launch frame by frame.
        const int want_group = t.seq_group > 0 ? t.seq_group : (on_device ? kSeqGroupDevice : kSeqGroupHost);
        G = (single || t.steps_path) ? 1 : std::min({want_group, n_slots, mpc::kFrameTable});
        return MPC_OK;
    }

    // the slot's frame is through: its container (and index) to the caller's arrays, or the call's first failure to `st`
    void collect(int slot) {
        Pending& p = pending[slot];
        if (p.frame < 0) return;
        const std::pair<uint8_t*, size_t> blob = p.result.get();
        if (st == MPC_OK && !blob.first) st = fail(MPC_ERR_HIP, "record download or container allocation failed");
        if (st == MPC_OK && index_interval) {                  // the slot's job holds the frame's index until the slot's next frame
            const std::vector<uint8_t>& index = jobs[slot].index;
            uint8_t* copy = index.empty() ? nullptr : static_cast<uint8_t*>(std::malloc(index.size()));
            if (!copy) {
                st = fail(MPC_ERR_ALLOC, "no seek index for frame %d", p.frame);
            } else {
                std::memcpy(copy, index.data(), index.size());
                indexes[p.frame] = copy;
                index_bytes[p.frame] = index.size();
            }
        }
        if (st == MPC_OK) {
            bytes[p.frame] = blob.first;
            nbytes[p.frame] = blob.second;
        } else {
            std::free(blob.first);
        }
        p.frame = -1;
    }

    // Host frames: frame g is copied into its slot's pinned image by a few threads and sent to the device while frame g - 1 is
    // still being enqueued and encoded; its pursuit waits for the event behind the copy.
    void start_upload(int g) {
        const int usl = g % n_slots;
        collect(usl);                     // the slot's previous frame is through
        uint8_t* d_img = reinterpret_cast<uint8_t*>(dev_slot_base(usl));
        uint8_t* pinned_rgb = reinterpret_cast<uint8_t*>(host_slot_base(usl));
        const uint8_t* src = frames[g];
        hipEvent_t ev_up = c->seq_events[usl][0];
        hipStream_t up_stream = c->seq_up;
        const int device = c->device;
        const size_t n = img_bytes;
        uploads[usl] = std::async(single ? std::launch::deferred : std::launch::async, [=]() -> hipError_t {
            // a 16 Mpixel frame: 48 MB staged at memcpy speed in 32 pieces, sent at PCIe speed behind them
            hipError_t e = staged_upload(device, src, pinned_rgb, d_img, 0, n, 32, up_stream);
            if (e == hipSuccess) e = hipSetDevice(device);
            if (e == hipSuccess) e = hipEventRecord(ev_up, up_stream);
            return e;
        });
    }

    // how far the pursuits may run ahead of the small kernels behind them: pursuit(f) waits for the stream assembly + phase 1
    // of frame f - lag_assembly and for the phase 2 of frame f - lag_phase2.  Measured (tools/ab_env_bench.sh, 4928x3264)
    // while the pursuits still filled every CU: lags 2 / 3 -> 4 660 Mpix/s, 3 / 3 -> 4 610 - 4 690, 3 / 4 -> 4 000 - 4 300,
    // 4 / 5 -> 4 090 - 4 680 (more slack let the chains of several frames pile up in front of one pursuit's end); with CUs
    // left free for the chains 2 / 2, 2 / 3 and 3 / 4 are within 1 % of each other.
    // The lags count launches: launch L = f / G covers the frames L * G ... (the last one of a call may be short).  A lag
    // that reaches back further than the slots do meets slots that were collected before: their events are old, the waits empty.
    mpc_status wait_for_lags(int launch) {
        for (int p = (launch - t.lag_phase2) * G; p >= 0 && p < (launch - t.lag_phase2 + 1) * G; ++p) {
            if (!phase2_enqueued[p % n_slots].valid()) continue;
            // frame p's phase 2 is on its slot's stream by now: this launch starts behind it (the event is the one
            // its worker recorded behind the container's copy; on the host route it is an old one and the wait is empty)
            phase2_enqueued[p % n_slots].get();
            HIP_TRY(hipStreamWaitEvent(pursuit_stream, c->seq_events[p % n_slots][2], 0));
        }
        for (int p = (launch - t.lag_assembly) * G; p >= 0 && p < (launch - t.lag_assembly + 1) * G; ++p)
            HIP_TRY(hipStreamWaitEvent(pursuit_stream, c->seq_events[p % n_slots][1], 0));
        return MPC_OK;
    }

    // One frame from host memory: nothing to overlap its upload with but its own tile encode.  The frame goes up in row
    // stripes and each stripe's tile encode starts behind its own copy (an event), writing its records where one launch
    // over the whole frame would put them: the copy of stripe s + 1 runs beside the encode of stripe s.
    mpc_status launch_striped(int f) {
        const int sl = f % n_slots;
        uint8_t* d_img = reinterpret_cast<uint8_t*>(dev_slot_base(sl));
        uint8_t* pinned_rgb = reinterpret_cast<uint8_t*>(host_slot_base(sl));
        mpc_basis_choice* d_choices = slot_choices(sl);
        HIP_TRY(hipMemsetAsync(d_choices, 0, sizeof(mpc_basis_choice) * n_tc * K, pursuit_stream));
        const size_t row_bytes = static_cast<size_t>(3) * width;
        for (int sp = 0; sp < single_stripes; ++sp) {
            const int rb = static_cast<int>(static_cast<long long>(tiles_y) * sp / single_stripes);
            const int re = static_cast<int>(static_cast<long long>(tiles_y) * (sp + 1) / single_stripes);
            const size_t lo = row_bytes * static_cast<size_t>(8 * rb), hi = row_bytes * static_cast<size_t>(std::min(height, 8 * re));
            HIP_TRY(staged_upload(c->device, frames[f], pinned_rgb, d_img, lo, hi, 8, c->seq_up));
            HIP_TRY(hipEventRecord(c->seq_stripe_up[sp], c->seq_up));
            HIP_TRY(hipStreamWaitEvent(pursuit_stream, c->seq_stripe_up[sp], 0));
            if (const mpc_status es = encode_batch_device(c, t, d_img, 1, 0, width, height, row_bytes, rb, re, quant, slot_counts(sl), d_choices,
                                                          nullptr, nullptr, pursuit_stream, true);
                es != MPC_OK)
                return es;
        }
        return MPC_OK;
    }

    // One pursuit launch over the frames f .. f + gn - 1.  Host frames: the launch waits for the uploads of all its frames.  The
    // uploads follow one another: the next one of the group starts as soon as one is through, the next group's first one behind
    // this group's launch (its slot's previous frame is the youngest still in flight; with one frame per launch, as ever, in
    // front of it)
    mpc_status launch_group(int f, int gn) {
        const int sl = f % n_slots;
        mpc::FrameTable table{};
        for (int k = 0; k < gn; ++k) {
            const int ks = (f + k) % n_slots;
            table.rgb[k] = frames[f + k];
            table.first[k] = static_cast<int>(ks * tiles);
            if (on_device) continue;
            HIP_TRY(uploads[ks].get());
            HIP_TRY(hipStreamWaitEvent(pursuit_stream, c->seq_events[ks][0], 0));
            if (f + k + 1 < n_frames && (k + 1 < gn || G == 1)) start_upload(f + k + 1);
            if (st != MPC_OK) return st;      // the frame that start_upload collected
            table.rgb[k] = reinterpret_cast<const uint8_t*>(dev_slot_base(ks));
        }
        table.n = gn;
        for (int k = gn; k < mpc::kFrameTable; ++k) { table.rgb[k] = table.rgb[0]; table.first[k] = table.first[0]; }
        if (single || t.steps_path)
            return encode_batch_device(c, t, table.rgb[0], 1, 0, width, height, static_cast<size_t>(3) * width, 0, tiles_y, quant,
                                       slot_counts(sl), slot_choices(sl), nullptr, nullptr, pursuit_stream, false);
        // the records beyond a tile-channel's count keep what an earlier frame left there: the stream assembly reads
        // min(count, K) of them (mp_streams.hip) and nothing else reads any
        return encode_batch_device(c, t, table.rgb[0], gn, 0, width, height, static_cast<size_t>(3) * width, 0, tiles_y, quant, slot_counts(0),
                                   slot_choices(0), nullptr, nullptr, pursuit_stream, false, &table);
    }

    // one event behind the launch; every frame's side stream waits for it, then runs the frame's container job
    mpc_status begin_containers(int f, int gn) {
        const int sl = f % n_slots;
        HIP_TRY(hipEventRecord(c->seq_pursuit_done[sl], pursuit_stream));
        for (int k = 0; k < gn; ++k) {
            const int fr = f + k, ks = fr % n_slots;
            ContainerJob& job = jobs[ks];
            job.side = c->seq_down[0];
            job.down = c->seq_down[1];
            job.phase1 = c->seq_events[ks][1];
            job.done = c->seq_events[ks][2];
            job.spin = single;
            job.host_stage = &c->host_stage;
            job.host_offset = ks * host_slot + route_at;
            job.index_interval = index_interval;
            job.index_expanded = index_expanded;
            HIP_TRY(hipStreamWaitEvent(job.side, c->seq_pursuit_done[sl], 0));
            if (const mpc_status bs = container_begin(job, c, t.host_entropy ? nullptr : &ent[ks], t.triple_limit, dev_slot_base(ks) + streams_at,
                                                      slot_counts(ks), reinterpret_cast<const uint32_t*>(slot_choices(ks)), nullptr, nullptr,
                                                      width, height, quant);
                bs != MPC_OK)
                return bs;
            auto told = std::make_shared<std::promise<void>>();
            phase2_enqueued[ks] = told->get_future();
            pending[ks].frame = fr;
            // the slot's worker: wait for the device, build the code tables, enqueue phase 2, collect the container
            const int device = c->device;
            const bool trace = t.trace;
            const double t_enq = trace_ms();
            ContainerJob* jp = &job;
            pending[ks].result = std::async(single ? std::launch::deferred : std::launch::async, [=]() -> std::pair<uint8_t*, size_t> {
                struct Tell {                                      // whatever happens, the enqueuing thread is released once
                    std::shared_ptr<std::promise<void>> p;
                    bool done = false;
                    void operator()() { if (!done) p->set_value(); done = true; }
                    ~Tell() { (*this)(); }
                } tell{told};
                std::pair<uint8_t*, size_t> blob{nullptr, 0};
                if (hipSetDevice(device) == hipSuccess && container_tables(*jp, [&] { tell(); }) == MPC_OK)
                    (void)container_collect(*jp, &blob.first, &blob.second);
                if (trace) {
                    const double* e = jp->stamps;
                    std::fprintf(stderr, "[trace] frame %d enqueued %.2f | device done %.2f | symbols on host %.2f | coded %.2f | entropy: stats %.2f tables %.2f bytes %.2f\n",
                                 fr, t_enq, e[0], jp->device_entropy ? e[4] : e[3], trace_ms(), e[1], e[2], e[4]);
                }
                return blob;
            });
        }
        return MPC_OK;
    }

    // the frame loop: stops on the first status that is not MPC_OK (a stage's, or a collected frame's in `st`)
    void encode_frames() {
        if (!on_device && !striped_single) start_upload(0);
        for (int f = 0, gn = 1; f < n_frames && st == MPC_OK; f += gn) {
            gn = std::min(G, n_frames - f);
            // frame f + k - slots is done with its slot: its download and its entropy stage have finished
            for (int k = 0; k < gn; ++k) collect((f + k) % n_slots);
            if (st == MPC_OK) st = wait_for_lags(f / G);
            if (st == MPC_OK) st = striped_single ? launch_striped(f) : launch_group(f, gn);
            if (st == MPC_OK) st = begin_containers(f, gn);
            if (st == MPC_OK && !on_device && !striped_single && G > 1 && f + gn < n_frames) start_upload(f + gn);
        }
    }

    // behind the frame loop, however it ended: nothing of the call is left on a thread or a stream, and a failed call returns nothing
    void drain() {
        for (auto& u : uploads)
            if (u.valid()) (void)u.get();
        for (int f = n_frames; f < n_frames + n_slots; ++f) collect(f % n_slots);   // oldest first
        (void)hipStreamSynchronize(c->seq_up);
        (void)hipStreamSynchronize(pursuit_stream);
        (void)hipStreamSynchronize(c->seq_down[0]);
        (void)hipStreamSynchronize(c->seq_down[1]);
        if (st != MPC_OK) {
            for (int f = 0; f < n_frames; ++f) { std::free(bytes[f]); bytes[f] = nullptr; nbytes[f] = 0; }
            if (index_interval)
                for (int f = 0; f < n_frames; ++f) { std::free(indexes[f]); indexes[f] = nullptr; index_bytes[f] = 0; }
        }
    }
};

// What every mpc_encode_image(s)* entry point is.  `interval`, `flags`: null where the entry point has no such argument.
mpc_status encode_sequence(mpc_context* c, const uint8_t* const* frames, bool on_device, int n_frames, int width, int height,
                           const double* quant, uint8_t** bytes, size_t* nbytes, const int* interval = nullptr,
                           const unsigned* flags = nullptr, uint8_t** indexes = nullptr, size_t* index_bytes = nullptr) {
    return guarded([&]() -> mpc_status {
    unsigned index_interval = 0;
    bool index_expanded = false;
    if (interval && (!indexes || !index_bytes)) return fail(MPC_ERR_ARGUMENT, "bad argument");
    if (interval)
        if (const mpc_status bad = index_interval_of(*interval, &index_interval)) return bad;
    if (flags)
        if (const mpc_status bad = index_flags_of(*flags, &index_expanded)) return bad;
    if (!c || !frames || !bytes || !nbytes || n_frames < 1) return fail(MPC_ERR_ARGUMENT, "bad argument");
    if (c->device < 0) return no_device();
    if (width < 1 || height < 1) return fail(MPC_ERR_ARGUMENT, "bad geometry");
    for (int f = 0; f < n_frames; ++f) {
        if (!frames[f]) return fail(MPC_ERR_ARGUMENT, "null frame");
        bytes[f] = nullptr;
        nbytes[f] = 0;
        if (index_interval) {
            indexes[f] = nullptr;
            index_bytes[f] = 0;
        }
    }
    const Tuning t = read_tuning();
    std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
    HIP_TRY(hipSetDevice(c->device));
    FramePipeline p{c, t, frames, on_device, n_frames, width, height, quant, bytes, nbytes, index_interval, indexes, index_bytes, index_expanded};
    if (const mpc_status ps = p.prepare(); ps != MPC_OK) return ps;
    {
        struct Drain {                                          // whichever way the frame loop is left
            FramePipeline& p;
            ~Drain() { p.drain(); }
        } on_every_exit{p};
        p.encode_frames();
    }
    return p.st;
    });
}
}  // namespace

extern "C" {

mpc_status mpc_encode_images(mpc_context* c, const uint8_t* const* rgb_frames, int n_frames, int width, int height,
                             const double* quant, uint8_t** bytes, size_t* nbytes) {
    return encode_sequence(c, rgb_frames, false, n_frames, width, height, quant, bytes, nbytes);
}

mpc_status mpc_encode_images_device(mpc_context* c, const uint8_t* const* d_rgb_frames, int n_frames, int width, int height,
                                    const double* quant, uint8_t** bytes, size_t* nbytes) {
    return encode_sequence(c, d_rgb_frames, true, n_frames, width, height, quant, bytes, nbytes);
}

// the same with every frame's seek index; n_frames == 1 is the single-frame route
mpc_status mpc_encode_images_indexed(mpc_context* c, const uint8_t* const* rgb_frames, int n_frames, int width, int height,
                                     const double* quant, int interval, uint8_t** bytes, size_t* nbytes, uint8_t** indexes,
                                     size_t* index_bytes) {
    return encode_sequence(c, rgb_frames, false, n_frames, width, height, quant, bytes, nbytes, &interval, nullptr, indexes, index_bytes);
}

mpc_status mpc_encode_images_indexed_device(mpc_context* c, const uint8_t* const* d_rgb_frames, int n_frames, int width, int height,
                                            const double* quant, int interval, uint8_t** bytes, size_t* nbytes, uint8_t** indexes,
                                            size_t* index_bytes) {
    return encode_sequence(c, d_rgb_frames, true, n_frames, width, height, quant, bytes, nbytes, &interval, nullptr, indexes, index_bytes);
}

// the two above with `flags`: 0 = the same call, MPC_INDEX_EXPANDED = every index is version 2 (mpc_container_index2's blob)
mpc_status mpc_encode_images_indexed2(mpc_context* c, const uint8_t* const* rgb_frames, int n_frames, int width, int height,
                                      const double* quant, int interval, unsigned flags, uint8_t** bytes, size_t* nbytes,
                                      uint8_t** indexes, size_t* index_bytes) {
    return encode_sequence(c, rgb_frames, false, n_frames, width, height, quant, bytes, nbytes, &interval, &flags, indexes, index_bytes);
}

mpc_status mpc_encode_images_indexed2_device(mpc_context* c, const uint8_t* const* d_rgb_frames, int n_frames, int width, int height,
                                             const double* quant, int interval, unsigned flags, uint8_t** bytes, size_t* nbytes,
                                             uint8_t** indexes, size_t* index_bytes) {
    return encode_sequence(c, d_rgb_frames, true, n_frames, width, height, quant, bytes, nbytes, &interval, &flags, indexes, index_bytes);
}

// compressed::encodeImage: one frame through the same stages
mpc_status mpc_encode_image(mpc_context* c, const uint8_t* rgb, int width, int height, const double* quant,
                            uint8_t** bytes, size_t* nbytes) {
    if (!rgb || !bytes || !nbytes) return fail(MPC_ERR_ARGUMENT, "null argument");
    return encode_sequence(c, &rgb, false, 1, width, height, quant, bytes, nbytes);
}

mpc_status mpc_encode_image_device(mpc_context* c, const uint8_t* d_rgb, int width, int height, const double* quant,
                                   uint8_t** bytes, size_t* nbytes) {
    if (!d_rgb || !bytes || !nbytes) return fail(MPC_ERR_ARGUMENT, "null argument");
    return encode_sequence(c, &d_rgb, true, 1, width, height, quant, bytes, nbytes);
}

}  // extern "C"
