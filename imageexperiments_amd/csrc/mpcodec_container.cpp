// mpcodec_container.cpp -- product: records on the device -> container bytes (ContainerJob: stream assembly, the entropy stage
// with its per-symbol work on the device, the host route) and the mpc_container_job_* API over it.  The frame pipeline
// (mpc_encode_image(s)[_device], mpcodec_pipeline.cpp) feeds it.
//
// Entropy stage (mp_entropy.hip): phase 1 is enqueued behind the stream assembly; the host then reads the per-stream statistics,
// builds the tables (host_bitstream.cpp: plan_stream), sends them back and enqueues phase 2, which writes the codes into the
// container on the device; only the finished bytes cross PCIe.  MPC_HOST_ENTROPY=1 keeps the whole stage on the host (the
// symbols cross instead); the same route is taken when a stream is outside what the device tables hold (more distinct symbols
// than the triple list, a code longer than 32 bits).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <utility>

#include <string>

#include "mpc_internal.h"

mpc_status entropy_buffers(EntropySlot& e, size_t tiles, int K, EntropyBuffers* b, int with_index) {
    const int S = 6 * K + 1;
    const size_t n_tc = 3 * tiles;
    const unsigned long long cap_symbols = n_tc + 2ULL * n_tc * K;
    const size_t blocks = mpc::entropy_max_blocks(cap_symbols, S);
    const size_t table_words = 65536 * static_cast<size_t>(S);          // dense code tables, histogram, first positions: [S][65536]
    const size_t out_bytes = Carve::up(sizeof(uint16_t) * 2 * n_tc * K) + 65536;
    const size_t max_cp = with_index ? mpc::entropy_max_checkpoints(cap_symbols, S) : 0;
    mpc::EntropyArgs& a = b->args;
    a = mpc::EntropyArgs{};
    b->h_checkpoints = nullptr;
    b->h_aux = nullptr;
    const bool with_aux = with_index == 2;                              // at most an entry per checkpoint: the same bound
    auto device_layout = [&](char* base) {
        Carve cv{base};
        a.streams = cv.take<mpc::EntStream>(S);
        a.totals = cv.take<unsigned>(4);
        for (unsigned** p : {&a.blk_stream, &a.blk_lead, &a.blk_inner, &a.blk_tail, &a.blk_carry, &a.blk_out, &a.blk_bits})
            *p = cv.take<unsigned>(blocks);
        a.blk_bit_off = cv.take<unsigned long long>(blocks);
        a.packed = cv.take<uint16_t>(2 * n_tc * K);
        a.tcode = cv.take<unsigned>(table_words);
        a.tlen = cv.take<uint8_t>(table_words);
        b->d_out = cv.take<uint8_t>(out_bytes);
        a.ghist = cv.take<unsigned>(table_words);
        a.gfirst = cv.take<unsigned>(table_words);
        if (with_index) a.checkpoints = cv.take<unsigned long long>(max_cp);
        if (with_aux) {
            a.aux = cv.take<unsigned long long>(2 * max_cp);
            a.aux_first = cv.take<unsigned>(S);
            a.blk_dc = cv.take<unsigned>(blocks);
        }
        return cv.at;
    };
    auto host_layout = [&](char* base) {
        Carve cv{base};
        b->h_streams = cv.take<mpc::EntStream>(S);
        b->h_totals = cv.take<unsigned>(4);
        b->h_triples = cv.take<unsigned>(3 * static_cast<size_t>(kTripleCap));
        b->h_entries = cv.take<unsigned>(3 * static_cast<size_t>(kTripleCap));
        b->h_out = cv.take<uint8_t>(out_bytes);
        if (with_index) b->h_checkpoints = cv.take<unsigned long long>(max_cp);
        if (with_aux) b->h_aux = cv.take<unsigned long long>(2 * max_cp);
        return cv.at;
    };
    bool grown = false;
    if (const mpc_status st = e.dev.reserve(device_layout(nullptr), "entropy stage buffers", &grown); st != MPC_OK) return st;
    if (const mpc_status st = e.host.reserve(host_layout(nullptr), "pinned entropy stage buffers"); st != MPC_OK) return st;
    if (grown) e.tiles = 0;
    device_layout(e.dev.data());
    host_layout(e.host.data());
    // the kernels read and write the small host-side tables in place (mapped, coherent host memory)
    char* mapped = nullptr;
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&mapped), e.host.p, 0));
    auto on_device = [&](void* h) { return mapped + (static_cast<char*>(h) - e.host.data()); };
    a.host_streams = reinterpret_cast<mpc::EntStream*>(on_device(b->h_streams));
    a.host_totals = reinterpret_cast<unsigned*>(on_device(b->h_totals));
    a.triples = reinterpret_cast<unsigned*>(on_device(b->h_triples));
    a.entries = reinterpret_cast<const unsigned*>(on_device(b->h_entries));
    a.n_lengths = static_cast<unsigned>(n_tc);
    a.n_streams = S;
    a.triple_cap = kTripleCap;
    a.out32 = reinterpret_cast<unsigned*>(b->d_out);
    a.cp_capacity = static_cast<unsigned>(max_cp);
    a.aux_capacity = with_aux ? static_cast<unsigned>(max_cp) : 0u;
    if (e.tiles != tiles || e.K != K) {
        // the dense code tables and the histogram are zero between frames (the kernels clear what they set), the first
        // positions all ones; a slot carved for another geometry holds them elsewhere
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemset(a.tcode, 0, sizeof(unsigned) * table_words));
        HIP_TRY(hipMemset(a.tlen, 0, table_words));
        HIP_TRY(hipMemset(a.ghist, 0, sizeof(unsigned) * table_words));
        HIP_TRY(hipMemset(a.gfirst, 0xFF, sizeof(unsigned) * table_words));
        e.tiles = tiles;
        e.K = K;
    }
    b->out_capacity = out_bytes;
    b->capacity_symbols = cap_symbols;
    return MPC_OK;
}

size_t host_route_layout(char* base, size_t n_tc, int K, HostRoute* r) {
    Carve cv{base};
    r->counts = cv.take<uint16_t>(n_tc);
    r->stream_off = cv.take<unsigned long long>(6 * static_cast<size_t>(K) + 1);
    r->symbols = cv.take<uint16_t>(2 * n_tc * K);
    return cv.at;
}

namespace {
enum class EntropyResult { kDone, kNeedsHost, kFailed };

// Wait for an event.  `spin`: poll it (a single frame's latency is a chain of such waits, and a sleeping thread takes tens of
// microseconds to come back); otherwise let the thread sleep -- in the frame pipeline the table building wants the cores.
hipError_t wait_event(hipEvent_t ev, bool spin) {
    if (!spin) return hipEventSynchronize(ev);
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        __builtin_ia32_pause();
    }
}

// The host's part and phase 2, in two steps.  Phase 1 has completed (the caller waited for an event behind it): the
// statistics are in the slot's host mirrors.
//   entropy_tables   builds the code tables and enqueues on `s`, in order: table import, the code kernels, the container's way
//                    to the host, `done`.  kNeedsHost: nothing enqueued, take the host route.
//   entropy_collect  waits for `done`, checks the device's bit counts against the tables', patches the host's pieces in.
EntropyResult entropy_tables(const EntropyBuffers& b, int device_block_size, int width, int height, int K, const double* quant,
                             unsigned triple_limit, unsigned index_interval, bool index_expanded, hipStream_t s, hipEvent_t done,
                             EntropyPending* pending, double* stamps) {
    const mpc::EntropyArgs& a = b.args;
    const int S = a.n_streams;
    if (b.h_totals[3] != 0 || b.h_totals[2] > triple_limit) return EntropyResult::kNeedsHost;
    stamps[0] = trace_ms();
    std::vector<mpc::StreamPlan>& plans = pending->plans;
    plans.assign(static_cast<size_t>(S), mpc::StreamPlan());
    std::vector<int> order(static_cast<size_t>(S));             // the streams with the most symbols to build a tree from first
    for (int j = 0; j < S; ++j) order[static_cast<size_t>(j)] = j;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return b.h_streams[x].distinct > b.h_streams[y].distinct; });
    mpc::parallel_jobs(S, [&](int job) {
        const int j = order[static_cast<size_t>(job)];
        const mpc::EntStream& st = b.h_streams[j];
        mpc::plan_stream(j != 0, st.shorter != 0, st.rle_size, st.eff_n, st.largest, b.h_triples + 3 * static_cast<size_t>(st.triple_off),
                         st.distinct, plans[static_cast<size_t>(j)]);
    });
    pending->head = mpc::container_head(width, height, K, device_block_size, quant);
    unsigned long long bit = pending->head.bit_size(), raw_symbols = 0;
    size_t n_entries = 0, n_cp = 0, n_aux = 0;
    if (index_interval && !(a.checkpoints && b.h_checkpoints)) return EntropyResult::kFailed;
    if (index_interval && index_expanded && !(a.aux && b.h_aux)) return EntropyResult::kFailed;
    for (int j = 0; j < S; ++j) {
        const mpc::StreamPlan& p = plans[static_cast<size_t>(j)];
        if (p.mode == 0 && p.max_code_length > 32) return EntropyResult::kNeedsHost;
        mpc::EntStream& st = b.h_streams[j];
        bit += p.pre.bit_size();
        st.bit_off = bit;
        st.mode = static_cast<unsigned>(p.mode);
        st.m = p.m;
        if (index_interval) {                                   // the stream's checkpoints: behind those of the streams before it
            st.reserved = static_cast<unsigned>(n_cp);
            const size_t chunks = (static_cast<size_t>(st.eff_n) + index_interval - 1) / index_interval;
            n_cp += chunks;
            // the aux entries phase 1 has left on the device: the same count the device derived (ent_aux_offsets_kernel)
            if (index_expanded && mpc::index_stream_has_aux(static_cast<size_t>(j), K, j != 0 && st.shorter != 0)) n_aux += chunks;
        }
        bit += p.payload_bits + p.post.bit_size();
        raw_symbols += st.n;
        n_entries += p.entries.size() / 3;
    }
    const size_t total_bytes = static_cast<size_t>((bit + 7) / 8), out_words = (total_bytes + 3) / 4;
    if (out_words * 4 > b.out_capacity || n_entries > kTripleCap || n_cp > a.cp_capacity) return EntropyResult::kNeedsHost;
    if (index_expanded && n_aux > a.aux_capacity) return EntropyResult::kNeedsHost;
    pending->total_bytes = total_bytes;
    pending->n_aux = n_aux;
    size_t at = 0;
    for (int j = 0; j < S; ++j) {
        const std::vector<uint32_t>& e = plans[static_cast<size_t>(j)].entries;
        for (size_t k = 0; k < e.size(); k += 3) {
            b.h_entries[at++] = (static_cast<unsigned>(j) << 16) | e[k];
            b.h_entries[at++] = e[k + 1];
            b.h_entries[at++] = e[k + 2];
        }
    }
    stamps[1] = trace_ms();                                     // tables built
    mpc::EntropyArgs a2 = a;
    a2.n_entries = static_cast<unsigned>(n_entries);
    a2.out_words = out_words;
    a2.cp_interval = index_interval;
    if (!index_interval) a2.checkpoints = nullptr;              // a slot carved for an index, a call without: the usual kernels
    const bool ok = hipMemsetAsync(b.d_out, 0, out_words * 4, s) == hipSuccess && mpc::launch_entropy_phase2(a2, raw_symbols, s) == 0 &&
                    hipMemcpyAsync(b.h_out, b.d_out, out_words * 4, hipMemcpyDeviceToHost, s) == hipSuccess &&
                    (n_cp == 0 || hipMemcpyAsync(b.h_checkpoints, a.checkpoints, sizeof(unsigned long long) * n_cp, hipMemcpyDeviceToHost,
                                                 s) == hipSuccess) &&
                    (n_aux == 0 || hipMemcpyAsync(b.h_aux, a.aux, 2 * sizeof(unsigned long long) * n_aux, hipMemcpyDeviceToHost, s) ==
                                       hipSuccess) &&
                    hipEventRecord(done, s) == hipSuccess;
    return ok ? EntropyResult::kDone : EntropyResult::kFailed;
}

EntropyResult entropy_collect(const EntropyBuffers& b, const EntropyPending& pending, const ContainerJob& job, hipEvent_t done, bool spin,
                              uint8_t** blob, size_t* nbytes, std::vector<uint8_t>* index, double* stamp) {
    if (wait_event(done, spin) != hipSuccess) return EntropyResult::kFailed;
    *stamp = trace_ms();                                        // codes written, bytes on the host
    const int S = b.args.n_streams;
    for (int j = 0; j < S; ++j)                                 // the device wrote exactly the bits the tables promise
        if (b.h_streams[j].coded_bits != pending.plans[static_cast<size_t>(j)].payload_bits) return EntropyResult::kFailed;
    mpc::or_bits(b.h_out, b.out_capacity, 0, pending.head);
    for (int j = 0; j < S; ++j) {
        const mpc::StreamPlan& p = pending.plans[static_cast<size_t>(j)];
        const unsigned long long payload = b.h_streams[j].bit_off;
        mpc::or_bits(b.h_out, b.out_capacity, static_cast<size_t>(payload - p.pre.bit_size()), p.pre);
        mpc::or_bits(b.h_out, b.out_capacity, static_cast<size_t>(payload + p.payload_bits), p.post);
    }
    if (job.index_interval) {
        // the index from what the stage holds: nothing of the container is parsed (host_container.cpp: index_from_plan)
        std::vector<mpc::PlannedStream> planned(static_cast<size_t>(S));
        for (int j = 0; j < S; ++j) {
            const mpc::EntStream& st = b.h_streams[j];
            mpc::PlannedStream& ps = planned[static_cast<size_t>(j)];
            ps.first_code_bit = st.bit_off;
            ps.n = st.n;
            ps.eff_n = st.eff_n;
            ps.shorter = st.shorter != 0;
        }
        if (!job.index_expanded) {
            if (!mpc::index_from_plan(job.index_interval, pending.total_bytes, job.width, job.height, job.K, job.block_size,
                                      pending.head.bit_size(), pending.plans.data(), planned.data(), S,
                                      reinterpret_cast<const uint64_t*>(b.h_checkpoints), *index))
                return EntropyResult::kFailed;
        } else if (!mpc::index_from_plan(job.index_interval, pending.total_bytes, job.width, job.height, job.K, job.block_size,
                                         pending.head.bit_size(), pending.plans.data(), planned.data(), S,
                                         reinterpret_cast<const uint64_t*>(b.h_checkpoints), *index, true,
                                         reinterpret_cast<const uint64_t*>(b.h_aux), pending.n_aux)) {
            // entries that contradict the plans: never a wrong blob -- the finished container is parsed instead.  MPC_INDEX_STRICT=1
            // (the device tests): an error, so that a kernel that writes such entries cannot hide behind the parse
            const char* strict = std::getenv("MPC_INDEX_STRICT");
            if (strict && std::atoi(strict) != 0) {
                std::fprintf(stderr, "[mpcodec] the device's aux entries contradict the stream plans (MPC_INDEX_STRICT)\n");
                return EntropyResult::kFailed;
            }
            if (!mpc::build_container_index(b.h_out, pending.total_bytes, job.index_interval, *index, true)) return EntropyResult::kFailed;
        }
    }
    uint8_t* out = static_cast<uint8_t*>(std::malloc(pending.total_bytes ? pending.total_bytes : 1));
    if (!out) return EntropyResult::kFailed;
    {   // fresh pages: a few threads fault them in and copy
        const size_t total = pending.total_bytes, piece = ((total + 7) / 8 + 4095) & ~static_cast<size_t>(4095);
        const uint8_t* src = b.h_out;
        mpc::parallel_jobs(total > (1u << 20) ? 8 : 1, [&](int k) {
            const size_t lo = std::min(total, piece * static_cast<size_t>(k));
            const size_t hi = total > (1u << 20) ? std::min(total, lo + piece) : total;
            if (hi > lo) std::memcpy(out + lo, src + lo, hi - lo);
        });
    }
    *blob = out;
    *nbytes = pending.total_bytes;
    return EntropyResult::kDone;
}

// the host route: the streams cross PCIe (unless they are on the host already), the entropy stage runs on the host (synchronous)
mpc_status container_on_host(ContainerJob& j) {
    const size_t n_tc = 3 * static_cast<size_t>(j.sa.tiles);
    const uint16_t* counts = j.h_counts;
    const unsigned long long* off = j.h_stream_off;
    const uint16_t* symbols = j.h_symbols;
    if (!counts) {
        HostRoute r;
        if (const mpc_status st = j.host_stage->reserve(j.host_offset + host_route_layout(nullptr, n_tc, j.K, &r), "pinned staging");
            st != MPC_OK)
            return st;
        host_route_layout(j.host_stage->data() + j.host_offset, n_tc, j.K, &r);
        const size_t n_off = 6 * static_cast<size_t>(j.K) + 1;
        HIP_TRY(hipMemcpyAsync(r.stream_off, j.sa.stream_off, sizeof(unsigned long long) * n_off, hipMemcpyDeviceToHost, j.down));
        HIP_TRY(hipMemcpyAsync(r.counts, j.sa.counts, sizeof(uint16_t) * n_tc, hipMemcpyDeviceToHost, j.down));
        HIP_TRY(hipEventRecord(j.done, j.down));
        HIP_TRY(hipEventSynchronize(j.done));
        const unsigned long long total = r.stream_off[n_off - 1];
        if (total > 2ULL * n_tc * static_cast<unsigned long long>(j.K)) return fail(MPC_ERR_HIP, "stream assembly returned an impossible size");
        if (total) HIP_TRY(hipMemcpyAsync(r.symbols, j.sa.symbols, sizeof(uint16_t) * total, hipMemcpyDeviceToHost, j.down));
        HIP_TRY(hipEventRecord(j.done, j.down));
        HIP_TRY(hipEventSynchronize(j.done));
        counts = r.counts;
        off = r.stream_off;
        symbols = r.symbols;
    }
    j.stamps[3] = trace_ms();
    j.blob = mpc::encode_symbol_streams_malloc(j.width, j.height, j.K, j.block_size, j.quant.data(), counts, symbols, off, &j.nblob);
    if (!j.blob) return fail(MPC_ERR_ALLOC, "out of memory");
    // the host route's index: the finished container parsed (rare; this is also where a "serial only" index comes from)
    if (j.index_interval && !mpc::build_container_index(j.blob, j.nblob, j.index_interval, j.index, j.index_expanded))
        return fail(MPC_ERR_BITSTREAM, "the container of the host route does not parse: no index");
    return MPC_OK;
}
}  // namespace

mpc_status container_begin(ContainerJob& j, const mpc_context* c, const EntropyBuffers* eb, unsigned triple_limit, char* buffers,
                           const uint16_t* d_counts, const uint32_t* d_choices, uint16_t* d_symbols,
                           unsigned long long* d_stream_off, int width, int height, const double* quant) {
    const long long tiles = static_cast<long long>((width + 7) / 8) * ((height + 7) / 8);
    j.width = width;
    j.height = height;
    j.K = c->K;
    j.block_size = c->block_size;
    const double* q = quant ? quant : c->quant.data();
    j.quant.assign(q, q + 3 * static_cast<size_t>(c->K));
    j.device_entropy = eb != nullptr;
    if (eb) j.eb = *eb;
    j.triple_limit = triple_limit;
    std::free(j.blob);
    j.blob = nullptr;
    j.nblob = 0;
    j.index.clear();
    mpc::StreamArgs& sa = j.sa;
    sa = mpc::StreamArgs{};
    sa.counts = d_counts;
    sa.choices = d_choices;
    if (buffers) {
        Carve cv{buffers};
        carve_stream_buffers(cv, tiles, c->K, true, &sa);
        if (const int err = mpc::launch_stream_assembly(sa, j.side); err != 0) return launch_failed(err);
    } else {
        sa.tiles = tiles;
        sa.K = c->K;
        sa.symbols = d_symbols;
        sa.stream_off = d_stream_off;
    }
    if (j.device_entropy) {
        j.eb.args.counts = d_counts;
        j.eb.args.symbols = sa.symbols;
        j.eb.args.stream_off = sa.stream_off;
        if (j.index_interval && j.index_expanded) {
            if (!j.eb.args.aux) return fail(MPC_ERR_ARGUMENT, "entropy buffers carved without the aux entries");
            j.eb.args.cp_interval = j.index_interval;           // the pack pass records the aux entries
        } else {
            j.eb.args.aux = nullptr;                            // a slot carved for them, a call without: the usual kernels
        }
        if (const int err = mpc::launch_entropy_phase1(j.eb.args, j.eb.capacity_symbols, j.side); err != 0) return launch_failed(err);
    }
    HIP_TRY(hipEventRecord(j.phase1, j.side));
    return MPC_OK;
}

mpc_status container_tables(ContainerJob& j, const std::function<void()>& enqueued) {
    if (wait_event(j.phase1, j.spin) != hipSuccess) return fail(MPC_ERR_HIP, "stream assembly or entropy phase 1 failed");
    j.stamps[0] = trace_ms();
    EntropyResult r = EntropyResult::kNeedsHost;
    if (j.device_entropy)
        r = entropy_tables(j.eb, j.block_size, j.width, j.height, j.K, j.quant.data(), j.triple_limit, j.index_interval, j.index_expanded, j.down,
                           j.done, &j.pending, j.stamps + 1);
    if (enqueued) enqueued();
    if (r == EntropyResult::kFailed) return fail(MPC_ERR_HIP, "device entropy stage failed: %s", hipGetErrorString(hipGetLastError()));
    if (r == EntropyResult::kDone) return MPC_OK;
    j.device_entropy = false;
    return container_on_host(j);
}

mpc_status container_collect(ContainerJob& j, uint8_t** bytes, size_t* nbytes) {
    if (!j.device_entropy) {
        *bytes = j.blob;
        *nbytes = j.nblob;
        j.blob = nullptr;
        j.nblob = 0;
        return MPC_OK;
    }
    const EntropyResult r = entropy_collect(j.eb, j.pending, j, j.done, j.spin, bytes, nbytes, &j.index, &j.stamps[4]);
    return r == EntropyResult::kDone ? MPC_OK : fail(MPC_ERR_HIP, "device entropy stage failed: %s", hipGetErrorString(hipGetLastError()));
}

// the `interval` argument of the indexed entry points as mpc_container_index takes it: 0 = the default
mpc_status index_interval_of(int interval, unsigned* out) {
    if (interval != 0 && (interval < static_cast<int>(mpc::kIndexIntervalMin) || interval > static_cast<int>(mpc::kIndexIntervalMax)))
        return fail(MPC_ERR_ARGUMENT, "interval %d: 0 or %u to %u", interval, mpc::kIndexIntervalMin, mpc::kIndexIntervalMax);
    *out = interval ? static_cast<unsigned>(interval) : mpc::kIndexIntervalDefault;
    return MPC_OK;
}

// the `flags` argument of the ...indexed2 entry points: MPC_INDEX_EXPANDED or nothing
mpc_status index_flags_of(unsigned flags, bool* expanded) {
    if (flags & ~MPC_INDEX_EXPANDED) return fail(MPC_ERR_ARGUMENT, "flags 0x%x: MPC_INDEX_EXPANDED or 0", flags);
    *expanded = (flags & MPC_INDEX_EXPANDED) != 0;
    return MPC_OK;
}

// records -> container on job slot 0 for a caller that waits, as a compose finishes, with the seek index from the entropy stage where
// one is asked for (`every` != 0; version 2, or version 1 without `expanded`).  The records and the geometry are the caller's: a whole
// frame's, or a packed frame's
mpc_status records_container(mpc_context* c, const Tuning& tuning, hipStream_t s, const uint16_t* d_counts, const mpc_basis_choice* d_choices,
                             long long tiles, int width, int height, const double* quant, unsigned every, ContainerMade* out, bool expanded) {
    const int K = c->K;
    if (!c->jobs[0]) c->jobs[0] = std::make_unique<JobSlot>();
    JobSlot& js = *c->jobs[0];
    ContainerJob& job = js.job;
    if (!job.phase1) {
        HIP_TRY(hipEventCreateWithFlags(&job.phase1, hipEventDisableTiming | hipEventBlockingSync));
        HIP_TRY(hipEventCreateWithFlags(&job.done, hipEventDisableTiming | hipEventBlockingSync));
    }
    Carve measure;
    mpc::StreamArgs measured{};
    carve_stream_buffers(measure, tiles, K, true, &measured);
    if (const mpc_status gs = js.dev.reserve(measure.at, "device staging"); gs != MPC_OK) return gs;
    GrowBuffer host_stage(GrowBuffer::kPinned);                 // the host route's, should the frame take it: this job's own
    job.side = job.down = s;
    job.spin = true;
    job.host_stage = &host_stage;
    job.host_offset = 0;
    job.index_interval = every;
    job.index_expanded = every != 0 && expanded;
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
        if (const mpc_status es = entropy_buffers(js.ent, static_cast<size_t>(tiles), K, &eb, every ? (expanded ? 2 : 1) : 0); es != MPC_OK) return es;
    HIP_TRY(hipStreamSynchronize(nullptr));                     // a slot carved for another geometry clears its tables on the null stream
    if (const mpc_status bs = container_begin(job, c, tuning.host_entropy ? nullptr : &eb, tuning.triple_limit, js.dev.data(), d_counts,
                                              reinterpret_cast<const uint32_t*>(d_choices), nullptr, nullptr, width, height, quant);
        bs != MPC_OK)
        return bs;
    if (const mpc_status ts = container_tables(job); ts != MPC_OK) return ts;
    uint8_t* made = nullptr;
    size_t made_bytes = 0;
    if (const mpc_status cs = container_collect(job, &made, &made_bytes); cs != MPC_OK) return cs;
    if (hipStreamSynchronize(s) != hipSuccess) {
        std::free(made);
        return fail(MPC_ERR_HIP, "the container job failed: %s", hipGetErrorString(hipGetLastError()));
    }
    if (every && job.index.empty()) {
        std::free(made);
        return fail(MPC_ERR_ALLOC, "no seek index");
    }
    std::free(out->bytes);
    out->bytes = made;
    out->nbytes = made_bytes;
    out->index.assign(job.index.begin(), job.index.end());
    return MPC_OK;
}

mpc_status deliver_container(ContainerMade& made, unsigned every, uint8_t** bytes, size_t* nbytes, uint8_t** index, size_t* index_bytes) {
    if (every) {
        uint8_t* copy = made.index.empty() ? nullptr : static_cast<uint8_t*>(std::malloc(made.index.size()));
        if (!copy) return fail(MPC_ERR_ALLOC, "no seek index");
        std::memcpy(copy, made.index.data(), made.index.size());
        *index = copy;
        *index_bytes = made.index.size();
    }
    *bytes = made.bytes;
    *nbytes = made.nbytes;
    made.bytes = nullptr;
    return MPC_OK;
}

namespace {
JobSlot* job_slot(mpc_context* c, int slot) {
    if (!c->jobs[slot]) c->jobs[slot] = std::make_unique<JobSlot>();
    return c->jobs[slot].get();
}

// mpc_code_symbol_streams_device[_indexed[2]]; index_interval != 0: with the container's seek index, version 2 if index_expanded
mpc_status code_symbol_streams(mpc_context* c, int width, int height, const double* quant, const uint16_t* counts, const uint16_t* symbols,
                               const unsigned long long* stream_off, unsigned index_interval, bool index_expanded, uint8_t** bytes,
                               size_t* nbytes, uint8_t** index, size_t* index_bytes, int* route) {
    return guarded([&]() -> mpc_status {
    if (!c || !counts || !stream_off || !bytes || !nbytes || width < 1 || height < 1) return fail(MPC_ERR_ARGUMENT, "bad argument");
    if (c->device < 0) return fail(MPC_ERR_NO_DEVICE, "context was created without a device");
    const int K = c->K;
    const size_t tiles = static_cast<size_t>((width + 7) / 8) * ((height + 7) / 8), n_tc = tiles * 3;
    for (int s = 0; s < 6 * K; ++s)
        if (stream_off[s + 1] < stream_off[s]) return fail(MPC_ERR_ARGUMENT, "stream offsets must not decrease");
    const unsigned long long total = stream_off[6 * K];
    if (stream_off[0] != 0 || total > 2ULL * n_tc * K || (total && !symbols)) return fail(MPC_ERR_ARGUMENT, "streams larger than a frame of this size can hold");
    if (index_interval) {
        *index = nullptr;
        *index_bytes = 0;
        if (!mpc::streams_match_lengths(counts, tiles, K, stream_off)) index_interval = 0;
    }
    const Tuning t = read_tuning();
    std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
    HIP_TRY(hipSetDevice(c->device));
    if (route) *route = 1;
    DeviceTemp d_counts, d_symbols, d_off;
    struct Job : ContainerJob {                                 // on the null stream; the host route codes the caller's streams
        ~Job() { if (phase1) (void)hipEventDestroy(phase1); if (done) (void)hipEventDestroy(done); }
    } j;
    j.h_counts = counts;
    j.h_stream_off = stream_off;
    j.h_symbols = symbols;
    j.index_interval = index_interval;
    j.index_expanded = index_expanded;
    HIP_TRY(hipEventCreateWithFlags(&j.phase1, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&j.done, hipEventDisableTiming));
    EntropyBuffers eb;
    if (!t.host_entropy) {
        if (const mpc_status es = entropy_buffers(c->ent[0], tiles, K, &eb, index_interval ? (index_expanded ? 2 : 1) : 0); es != MPC_OK)
            return es;
        const size_t n_off = 6 * static_cast<size_t>(K) + 1;
        HIP_TRY(hipMalloc(&d_counts.p, sizeof(uint16_t) * n_tc));
        HIP_TRY(hipMalloc(&d_symbols.p, sizeof(uint16_t) * (total ? total : 1)));
        HIP_TRY(hipMalloc(&d_off.p, sizeof(unsigned long long) * n_off));
        HIP_TRY(hipMemcpy(d_counts.p, counts, sizeof(uint16_t) * n_tc, hipMemcpyHostToDevice));
        if (total) HIP_TRY(hipMemcpy(d_symbols.p, symbols, sizeof(uint16_t) * total, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_off.p, stream_off, sizeof(unsigned long long) * n_off, hipMemcpyHostToDevice));
    }
    mpc_status st = container_begin(j, c, t.host_entropy ? nullptr : &eb, t.triple_limit, nullptr, static_cast<const uint16_t*>(d_counts.p),
                                    nullptr, static_cast<uint16_t*>(d_symbols.p), static_cast<unsigned long long*>(d_off.p), width, height,
                                    quant);
    if (st == MPC_OK) st = container_tables(j);
    if (st == MPC_OK) st = container_collect(j, bytes, nbytes);
    if (st == MPC_OK && index_interval) {
        uint8_t* copy = j.index.empty() ? nullptr : static_cast<uint8_t*>(std::malloc(j.index.size()));
        if (copy) {
            std::memcpy(copy, j.index.data(), j.index.size());
            *index = copy;
            *index_bytes = j.index.size();
        } else {
            std::free(*bytes);
            *bytes = nullptr;
            *nbytes = 0;
            st = fail(MPC_ERR_ALLOC, "no seek index");
        }
    }
    if (st == MPC_OK && route && j.device_entropy) *route = 0;
    HIP_TRY(hipDeviceSynchronize());
    return st;
    });
}
}  // namespace

extern "C" {

// ---- records that are already on the device in whole-frame order -> container (the owner of a frame in the multi-GPU path,
// after the stripe exchange; the rate-distortion sweep), in three steps so that the caller can keep the device busy meanwhile:
//   begin    stream assembly + entropy phase 1 enqueued on `stream`; nothing is waited for
//   tables   waits for phase 1, builds the code tables, enqueues phase 2 and the container's copy on the same stream
//   collect  waits for the copy; the container
// One job per slot at a time.  mpc_records_to_container_device is the three in a row on slot 0.
mpc_status mpc_container_job_begin(mpc_context* c, int slot, const uint16_t* d_counts, const mpc_basis_choice* d_choices, int width,
                                   int height, const double* quant, void* stream) {
    return guarded([&]() -> mpc_status {
    if (!c || !d_counts || !d_choices || slot < 0 || slot >= mpc_context::kSeqSlots) return fail(MPC_ERR_ARGUMENT, "bad argument");
    if (c->device < 0) return fail(MPC_ERR_NO_DEVICE, "context was created without a device");
    if (width < 1 || height < 1) return fail(MPC_ERR_ARGUMENT, "bad geometry");
    const Tuning t = read_tuning();
    const long long tiles = static_cast<long long>((width + 7) / 8) * ((height + 7) / 8);
    std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
    HIP_TRY(hipSetDevice(c->device));
    if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
    JobSlot* js = job_slot(c, slot);
    if (js->stage != 0) return fail(MPC_ERR_ARGUMENT, "container job slot %d is busy", slot);
    Carve measure;
    mpc::StreamArgs measured{};
    carve_stream_buffers(measure, tiles, c->K, true, &measured);
    if (const mpc_status gs = js->dev.reserve(measure.at, "device staging"); gs != MPC_OK) return gs;
    ContainerJob& j = js->job;
    if (!j.phase1) {
        HIP_TRY(hipEventCreateWithFlags(&j.phase1, hipEventDisableTiming | hipEventBlockingSync));
        HIP_TRY(hipEventCreateWithFlags(&j.done, hipEventDisableTiming | hipEventBlockingSync));
    }
    j.side = j.down = static_cast<hipStream_t>(stream);
    j.host_stage = &c->host_stage;
    EntropyBuffers eb;
    if (!t.host_entropy)
        if (const mpc_status es = entropy_buffers(js->ent, static_cast<size_t>(tiles), c->K, &eb); es != MPC_OK) return es;
    const mpc_status st = container_begin(j, c, t.host_entropy ? nullptr : &eb, t.triple_limit, js->dev.data(), d_counts,
                                          reinterpret_cast<const uint32_t*>(d_choices), nullptr, nullptr, width, height, quant);
    if (st == MPC_OK) js->stage = 1;
    return st;
    });
}

mpc_status mpc_container_job_tables(mpc_context* c, int slot) {
    return guarded([&]() -> mpc_status {
    if (!c || slot < 0 || slot >= mpc_context::kSeqSlots) return fail(MPC_ERR_ARGUMENT, "bad argument");
    std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
    JobSlot* js = job_slot(c, slot);
    if (js->stage != 1) return fail(MPC_ERR_ARGUMENT, "container job slot %d has not begun", slot);
    HIP_TRY(hipSetDevice(c->device));
    const mpc_status st = container_tables(js->job);
    js->stage = st == MPC_OK ? 2 : 0;
    return st;
    });
}

mpc_status mpc_container_job_collect(mpc_context* c, int slot, uint8_t** bytes, size_t* nbytes) {
    return guarded([&]() -> mpc_status {
    if (!c || !bytes || !nbytes || slot < 0 || slot >= mpc_context::kSeqSlots) return fail(MPC_ERR_ARGUMENT, "bad argument");
    std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
    JobSlot* js = job_slot(c, slot);
    if (js->stage != 2) return fail(MPC_ERR_ARGUMENT, "container job slot %d has no tables yet", slot);
    HIP_TRY(hipSetDevice(c->device));
    js->stage = 0;
    return container_collect(js->job, bytes, nbytes);
    });
}

mpc_status mpc_container_job_cancel(mpc_context* c, int slot) {
    return guarded([&]() -> mpc_status {
    if (!c || slot < 0 || slot >= mpc_context::kSeqSlots) return fail(MPC_ERR_ARGUMENT, "bad argument");
    std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
    if (!c->jobs[slot]) return MPC_OK;
    JobSlot* js = job_slot(c, slot);
    if (js->stage != 0 && c->device >= 0) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(js->job.side));       // whatever the job has enqueued has left its buffers
    }
    std::free(js->job.blob);
    js->job.blob = nullptr;
    js->job.nblob = 0;
    js->stage = 0;
    return MPC_OK;
    });
}

mpc_status mpc_interleave_stripe_device(mpc_context* c, const uint16_t* d_part_counts, const mpc_basis_choice* d_part_choices, int width,
                                        int height, int tile_row_begin, int tile_row_end, uint16_t* d_frame_counts,
                                        mpc_basis_choice* d_frame_choices, void* stream) {
    if (!c || !d_part_counts || !d_part_choices || !d_frame_counts || !d_frame_choices) return fail(MPC_ERR_ARGUMENT, "null argument");
    if (c->device < 0) return fail(MPC_ERR_NO_DEVICE, "context was created without a device");
    if (width < 1 || height < 1) return fail(MPC_ERR_ARGUMENT, "bad geometry");
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    if (tile_row_begin < 0 || tile_row_end > tiles_y || tile_row_begin >= tile_row_end)
        return fail(MPC_ERR_ARGUMENT, "tile rows [%d,%d) outside 0..%d", tile_row_begin, tile_row_end, tiles_y);
    HIP_TRY(hipSetDevice(c->device));
    if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
    const int err = mpc::launch_interleave_stripe(d_part_counts, reinterpret_cast<const uint32_t*>(d_part_choices), tiles_x, tiles_y, tile_row_begin,
                                                  tile_row_end - tile_row_begin, c->K, d_frame_counts, reinterpret_cast<uint32_t*>(d_frame_choices), stream);
    if (err != 0) return launch_failed(err);
    return MPC_OK;
}

// the context's crop error word, made on first use (the device is current)
mpc_status crop_flag(mpc_context* c) {
    if (c->d_crop_flag) return MPC_OK;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->d_crop_flag), sizeof(int)));
    HIP_TRY(hipMemset(c->d_crop_flag, 0, sizeof(int)));
    HIP_TRY(hipDeviceSynchronize());
    return MPC_OK;
}

mpc_status mpc_crop_records_device(mpc_context* c, const uint16_t* d_counts, const mpc_basis_choice* d_choices, int width, int height,
                                   const mpc_rect* rect, int steps, uint16_t* d_out_counts, mpc_basis_choice* d_out_choices, void* stream) {
    return guarded([&]() -> mpc_status {
    if (!c || !d_counts || !d_choices || !rect || !d_out_counts || !d_out_choices) return fail(MPC_ERR_ARGUMENT, "null argument");
    if (c->device < 0) return fail(MPC_ERR_NO_DEVICE, "context was created without a device");
    if (steps < 0) return fail(MPC_ERR_ARGUMENT, "steps must not be negative");
    if (width < 1 || height < 1) return fail(MPC_ERR_ARGUMENT, "bad geometry");
    const mpc_rect r = rect->x == 0 && rect->y == 0 && rect->width == 0 && rect->height == 0 ? mpc_rect{0, 0, width, height} : *rect;
    const std::string why = mpc::transcode_rect_error(width, height, c->block_size, r.x, r.y, r.width, r.height);
    if (!why.empty()) return fail(MPC_ERR_ARGUMENT, "%s", why.c_str());
    mpc::TileWindow win;
    mpc::tile_window(width, height, c->block_size, r.x, r.y, r.width, r.height, win);
    HIP_TRY(hipSetDevice(c->device));
    if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
    if (const mpc_status fs = crop_flag(c); fs != MPC_OK) return fs;
    const int bs = c->block_size;
    const int err = mpc::launch_crop_records(d_counts, reinterpret_cast<const uint32_t*>(d_choices), (width + bs - 1) / bs, win.tiles_y, win.tx0,
                                             win.ty0, win.tx1, win.ty1, c->K, steps > 0 && steps < c->K ? steps : c->K, d_out_counts,
                                             reinterpret_cast<uint32_t*>(d_out_choices), c->d_crop_flag, stream);
    if (err != 0) return launch_failed(err);
    return MPC_OK;
    });
}

mpc_status mpc_paste_records_device(mpc_context* c, const uint16_t* d_src_counts, const mpc_basis_choice* d_src_choices, int src_width,
                                    int src_height, const mpc_rect* src_rect, uint16_t* d_dst_counts, mpc_basis_choice* d_dst_choices,
                                    int dst_width, int dst_height, int dst_x, int dst_y, const int32_t* d_owner, int part, void* stream) {
    return guarded([&]() -> mpc_status {
    if (!c || !d_src_counts || !d_src_choices || !src_rect || !d_dst_counts || !d_dst_choices) return fail(MPC_ERR_ARGUMENT, "null argument");
    if (c->device < 0) return fail(MPC_ERR_NO_DEVICE, "context was created without a device");
    if (src_width < 1 || src_height < 1 || dst_width < 1 || dst_height < 1) return fail(MPC_ERR_ARGUMENT, "bad geometry");
    const int bs = c->block_size;
    mpc::ComposePart piece;
    const bool whole = src_rect->x == 0 && src_rect->y == 0 && src_rect->width == 0 && src_rect->height == 0;
    piece.x = src_rect->x;
    piece.y = src_rect->y;
    piece.w = whole ? src_width : src_rect->width;
    piece.h = whole ? src_height : src_rect->height;
    piece.dx = dst_x;
    piece.dy = dst_y;
    piece.src_width = src_width;
    piece.src_height = src_height;
    const std::string why = mpc::compose_part_error(piece, bs, dst_width, dst_height);
    if (!why.empty()) return fail(MPC_ERR_ARGUMENT, "%s", why.c_str());
    const long long dst_tiles_x = (static_cast<long long>(dst_width) + bs - 1) / bs, dst_tiles_y = (static_cast<long long>(dst_height) + bs - 1) / bs;
    if (dst_tiles_x * dst_tiles_y >= (1LL << 31)) return fail(MPC_ERR_ARGUMENT, "bad geometry");
    HIP_TRY(hipSetDevice(c->device));
    if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
    if (const mpc_status fs = crop_flag(c); fs != MPC_OK) return fs;
    const int stx0 = piece.x / bs, sty0 = piece.y / bs;
    const int err = mpc::launch_paste_records(d_src_counts, reinterpret_cast<const uint32_t*>(d_src_choices), (src_width + bs - 1) / bs,
                                              (src_height + bs - 1) / bs, stx0, sty0, (piece.x + piece.w + bs - 1) / bs - stx0,
                                              (piece.y + piece.h + bs - 1) / bs - sty0, c->K, d_dst_counts, reinterpret_cast<uint32_t*>(d_dst_choices),
                                              static_cast<int>(dst_tiles_x), static_cast<int>(dst_tiles_y), dst_x / bs, dst_y / bs, d_owner, part,
                                              c->d_crop_flag, stream);
    if (err != 0) return launch_failed(err);
    return MPC_OK;
    });
}

mpc_status mpc_crop_records_check(mpc_context* c, void* stream) {
    return guarded([&]() -> mpc_status {
    if (!c) return fail(MPC_ERR_ARGUMENT, "null context");
    if (c->device < 0) return fail(MPC_ERR_NO_DEVICE, "context was created without a device");
    if (!c->d_crop_flag) return MPC_OK;                             // nothing has been cropped yet
    HIP_TRY(hipSetDevice(c->device));
    if (const mpc_status cs = refuse_capture(stream); cs != MPC_OK) return cs;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, c->d_crop_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemsetAsync(c->d_crop_flag, 0, sizeof(int), s));
    HIP_TRY(hipStreamSynchronize(s));
    return flag ? fail(MPC_ERR_BITSTREAM, "Invalid bitstream") : MPC_OK;
    });
}

mpc_status mpc_records_to_container_device(mpc_context* c, const uint16_t* d_counts, const mpc_basis_choice* d_choices, int width,
                                           int height, const double* quant, void* stream, uint8_t** bytes, size_t* nbytes) {
    if (!bytes || !nbytes) return fail(MPC_ERR_ARGUMENT, "null argument");
    if (!c) return fail(MPC_ERR_ARGUMENT, "null context");
    std::lock_guard<std::recursive_mutex> one_host_call(c->host_calls);
    mpc_status st = mpc_container_job_begin(c, 0, d_counts, d_choices, width, height, quant, stream);
    if (st == MPC_OK) st = mpc_container_job_tables(c, 0);
    if (st == MPC_OK) st = mpc_container_job_collect(c, 0, bytes, nbytes);
    return st;
}

// The entropy stage alone, on streams the caller holds in host memory (what mpc_assemble_symbol_streams codes on the host):
// upload, device entropy stage, container bytes.  *route (optional): 0 = coded on the device, 1 = the host route was taken.
mpc_status mpc_code_symbol_streams_device(mpc_context* c, int width, int height, const double* quant, const uint16_t* counts,
                                          const uint16_t* symbols, const unsigned long long* stream_off, uint8_t** bytes, size_t* nbytes,
                                          int* route) {
    return code_symbol_streams(c, width, height, quant, counts, symbols, stream_off, 0, false, bytes, nbytes, nullptr, nullptr, route);
}

// The same with the container's seek index.  Streams that do not hold what `counts` implies (only a test makes such) give a
// container no parser accepts: it comes back alone, *index = NULL.
mpc_status mpc_code_symbol_streams_device_indexed(mpc_context* c, int width, int height, const double* quant, const uint16_t* counts,
                                                  const uint16_t* symbols, const unsigned long long* stream_off, int interval,
                                                  uint8_t** bytes, size_t* nbytes, uint8_t** index, size_t* index_bytes, int* route) {
    unsigned every = 0;
    if (!index || !index_bytes) return fail(MPC_ERR_ARGUMENT, "bad argument");
    if (const mpc_status bad = index_interval_of(interval, &every)) return bad;
    return code_symbol_streams(c, width, height, quant, counts, symbols, stream_off, every, false, bytes, nbytes, index, index_bytes, route);
}

// flags 0: the call above; MPC_INDEX_EXPANDED: *index is the version-2 blob mpc_container_index2 builds from the container
mpc_status mpc_code_symbol_streams_device_indexed2(mpc_context* c, int width, int height, const double* quant, const uint16_t* counts,
                                                   const uint16_t* symbols, const unsigned long long* stream_off, int interval,
                                                   unsigned flags, uint8_t** bytes, size_t* nbytes, uint8_t** index, size_t* index_bytes,
                                                   int* route) {
    unsigned every = 0;
    bool expanded = false;
    if (!index || !index_bytes) return fail(MPC_ERR_ARGUMENT, "bad argument");
    if (const mpc_status bad = index_interval_of(interval, &every)) return bad;
    if (const mpc_status bad = index_flags_of(flags, &expanded)) return bad;
    return code_symbol_streams(c, width, height, quant, counts, symbols, stream_off, every, expanded, bytes, nbytes, index, index_bytes,
                               route);
}

}  // extern "C"
