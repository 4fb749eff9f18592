// mp_parse.hip -- product: the decoder's entropy codes undone on the device, in front of mp_unpack.hip: what the host's serial
// parse (mpc::read_compressed_coded) is to the serial route.
//
// Input: the container's bytes as they are, and a seek index the host has checked against them (host_container.cpp:
// plan_indexed_parse): for every one of the 1 + 6K streams the bit of every `interval`-th code (a checkpoint) and the bit behind the
// stream.  Output: the coded streams where launch_unpack reads them (UnpackArgs::coded, UnpackStream layout) and the lengths
// where the gather and the reconstruction read them (`counts`).
//
//   parse    one wave per group of 64 consecutive chunks of one stream, a lane per chunk.  A lane decodes its chunk's codes from its
//            checkpoint with the serial parser's decisions exactly (huffman_step / golomb_step of host_bitstream.cpp): the first
//            (shortest) length at which the next bits are a code of that length -- an 11-bit window table in LDS, filled by the host
//            shortest length first, longer codes by the per-length test in order of length; Golomb with the remainder in
//            bit_width(M) bits, the `limit` escape and unary runs of any length.
//   hist / verify / void   the sizes the decoded lengths give the 6K streams, compared with the index's; if they differ every
//            length is zeroed, so that the gather -- which lays the streams out by the lengths, not by the host's table -- reads
//            nothing
//
// Shape (cdna_hip_programming.md): a stream's codes chain bit to bit, so the parallelism is chunks, and a chunk is a lane.  The
// lanes of a wave share a stream, hence one code table (LDS, 8 KB) and one branch between Huffman and Golomb per wave; the loop
// over symbols has the same trip count in every lane and only the long-code path and long unary runs diverge.  A lane's bits come
// through a 64-bit register window refilled by aligned 4-byte loads: consecutive loads of a lane fall into one cache line, which
// L1/L2 serve.  The 64 chunks' output is contiguous, so symbols are staged in LDS, a padded row per lane (17 words: a lane's
// writes and the 16-lane row reads hit distinct banks), and leave as aligned 4-byte words, 64 bytes a row (mp_unpack_fill_kernel's
// way) instead of 64 scattered 2-byte stores.  One wave per workgroup: waves share nothing, and 12.25 KB of LDS
// admits 13 of them on a CU, three to four a SIMD (the resource report's 4).
//
// The input is untrusted, the index included.  Every bound below comes from the host's tables (ParseStream, checkpoints): a lane
// reads bits in [checkpoint, required end), where required end <= 8 * the container's bytes, and the buffer is zero-padded 16 bytes
// beyond; it writes symbols [chunk * interval, + min(interval, n_coded - chunk * interval)) of its stream and nothing else.  A lane
// whose next code would pass its required end stops, writes zeros for the rest and sets the error word; so does one that ends
// short of it.  The host then decodes the frame by the serial route, whose verdict is the caller's.  Nothing is indexed by a
// decoded value except the entry -> symbol table, with an entry the host's per-length table bounds by `total`.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mp_device.h"
#include "mp_codes.h"

namespace mpc {

namespace {
constexpr int kTile = 32;                       // symbols a lane stages between two write-outs
constexpr int kRow = kTile + 2;                 // u16 per staged row: 17 words
constexpr int kLutSize = 1 << kParseLutBits;
constexpr int kHistRow = kMaxDeviceK + 1;
constexpr int kSizesDiffer = 3 * kHistRow;      // hist[kSizesDiffer]: the verify kernel's verdict

// the stream group `g` belongs to: the last one whose first group is not behind g.  streams[n_streams].group_begin = n_groups > g
__device__ __forceinline__ int stream_of_group(const ParseArgs& a, unsigned g) {
    int lo = 0, hi = a.n_streams;                                   // invariant: streams[lo].group_begin <= g < streams[hi].group_begin
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.streams[mid].group_begin <= g) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace

// kWindow (launch_parse_window): the grid is the 6K streams' groups, the first of them a.group_first, and of stream s only the
// chunks [c0, c1) of a.window[s - 1] are wanted (mp_window_rank_kernel wrote them, cut to the stream's chunks; they are cut again
// here).  A group that holds none of them leaves before it fills its table; in a group that straddles the range the chunks outside
// it are what chunks behind the stream's last are: no lane reads them, no row of theirs is written.  Positions are the whole
// frame's, so the symbols of unparsed chunks are simply never written.
template <bool kWindow>
__global__ __launch_bounds__(64) void mp_parse_kernel(const ParseArgs a)
{
    __shared__ uint32_t lut[kLutSize];
    __shared__ uint16_t stage[kParseGroup * kRow];
    const unsigned g = kWindow ? blockIdx.x + a.group_first : blockIdx.x;     // < n_groups (the grid)
    const int lane = threadIdx.x;
    const int si = stream_of_group(a, g);
    const ParseStream st = a.streams[si];
    const bool golomb = (st.flags & kParseGolomb) != 0u, lengths = (st.flags & kParseLengths) != 0u;
    const unsigned long long interval = a.interval;
    const unsigned long long j0 = (unsigned long long)(g - st.group_begin) * kParseGroup;     // < n_chunks: the stream has ceil(n_chunks / 64) groups
    unsigned long long c0 = 0, c1 = st.n_chunks;
    if (kWindow) {                                                  // group_first = streams[1].group_begin: si >= 1
        const WindowStream win = a.window[si - 1];
        c0 = win.c0;
        c1 = win.c1 < st.n_chunks ? win.c1 : st.n_chunks;
        if (j0 + kParseGroup <= c0 || j0 >= c1) return;             // the whole wave
    }
    // chunk j of the stream: symbols [j * interval, j * interval + rows(j))
    auto symbols_of = [&](unsigned long long j) -> unsigned {
        if (j >= c1 || j < c0) return 0u;
        const unsigned long long rest = st.n_coded - j * interval;  // > 0: n_chunks = ceil(n_coded / interval)
        return (unsigned)(rest < interval ? rest : interval);
    };
    const unsigned long long j = j0 + lane;
    const bool active = j >= c0 && j < c1;
    const bool last = active && j + 1 == st.n_chunks;
    const unsigned n = symbols_of(j);
    if (!golomb) {
        // lut_off + kLutSize lies inside `luts`: the host lays one whole table out per Huffman stream
        const uint4* src = reinterpret_cast<const uint4*>(a.luts + st.lut_off);
        for (int i = lane; i < kLutSize / 4; i += 64) reinterpret_cast<uint4*>(lut)[i] = src[i];
    }
    Bits in;
    {
        // cp_off + j, cp_off + j + 1 < cp_off + n_chunks: the stream's own checkpoints
        const unsigned long long begin = active ? a.checkpoints[st.cp_off + j] : 0ull;
        const unsigned long long end = !active ? 0ull : last ? st.end_bit : a.checkpoints[st.cp_off + j + 1];
        in.open(a.words, begin, end < begin ? begin : end);         // the host has ordered them; a lane never trusts that
    }
    const unsigned b = golomb ? 32u - (unsigned)__clz((int)st.m) : 0u;                          // bit_width(M), M >= 1
    const unsigned limit = golomb ? (1u << (b + 1u)) - st.m : 0u;
    bool bad = false, beyond_k = false;
    __syncthreads();
    const unsigned n_first = symbols_of(j0 < c0 ? c0 : j0);           // the group's longest chunk: only a stream's last one is shorter
    uint16_t* const out = lengths ? a.counts : a.coded;
    for (unsigned t0 = 0; t0 < n_first; t0 += kTile) {
        for (unsigned t = 0; t < (unsigned)kTile; ++t) {
            unsigned v = 0;
            if (t0 + t < n && !bad) {
                if (golomb) bad = !golomb_one(st.m, b, limit, in, &v);
                else bad = huffman_one(a, st, lut, in, &v) != 0;
                if (bad) v = 0;
                v &= 0xFFFFu;
                if (lengths && v > (unsigned)a.K) {                 // what follows indexes by it: cut it, and say so
                    v = (unsigned)a.K;
                    beyond_k = true;
                }
            }
            stage[lane * kRow + t] = (uint16_t)v;                   // t < kTile < kRow
        }
        __syncthreads();
        // 16 lanes a row, 4 rows a pass: row r = chunk j0 + r, its symbols [t0, t0 + kTile) that exist, as aligned words
        for (int pass = 0; pass < kParseGroup / 4; ++pass) {
            const int r = pass * 4 + (lane >> 4), sub = lane & 15;
            const unsigned rows = symbols_of(j0 + r);
            const unsigned have = rows > t0 ? (rows - t0 < (unsigned)kTile ? rows - t0 : (unsigned)kTile) : 0u;
            // [e0, e1) lies inside the stream's [out_off, out_off + n_coded), which the host placed inside the buffer
            const unsigned long long e0 = st.out_off + (j0 + r) * interval + t0, e1 = e0 + have;
            for (unsigned long long w = (e0 >> 1) + sub; 2 * w < e1; w += 16) {                 // at most 17 words: two rounds
                const unsigned long long e = 2 * w;
                const bool lo = e >= e0, hi = e + 1 < e1;           // e < e1 (the loop), e + 1 >= e0 (w >= e0 / 2)
                const uint16_t vlo = lo ? stage[r * kRow + (int)(e - e0)] : (uint16_t)0;       // e - e0 < have <= kTile
                const uint16_t vhi = hi ? stage[r * kRow + (int)(e + 1 - e0)] : (uint16_t)0;
                if (lo && hi) reinterpret_cast<uint32_t*>(out)[w] = (uint32_t)vlo | ((uint32_t)vhi << 16);
                else if (lo) out[e] = vlo;
                else if (hi) out[e + 1] = vhi;
            }
        }
        __syncthreads();
    }
    if (active && !bad) {
        if (last && !golomb) {                                      // the pseudo-EOF closes a Huffman stream
            unsigned none;
            bad = huffman_one(a, st, lut, in, &none) != 1;
        }
        bad = bad || in.left != 0ull;                               // exactly on the next checkpoint / the stream's end
    }
    if (bad || beyond_k) atomicOr(a.error, 1);
}

// the lengths' histogram per channel (every length is <= K: the parse kernel cut them)
__global__ __launch_bounds__(256) void mp_parse_hist_kernel(const ParseArgs a)
{
    __shared__ unsigned hist[3 * kHistRow];
    for (int i = threadIdx.x; i < 3 * kHistRow; i += 256) hist[i] = 0;
    __syncthreads();
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < a.n_counts; i += (unsigned long long)gridDim.x * 256) {
        const unsigned c = a.counts[i];
        atomicAdd(&hist[(unsigned)(i % 3) * kHistRow + (c < (unsigned)a.K ? c : (unsigned)a.K)], 1u);     // <= K <= kMaxDeviceK
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * kHistRow; i += 256)
        if (hist[i]) atomicAdd(&a.hist[i], hist[i]);
}

// stream sizes from the histogram (CompressedImage.cpp:680-685) against the index's
__global__ __launch_bounds__(128) void mp_parse_verify_kernel(const ParseArgs a)
{
    const int i = threadIdx.x;                                      // (channel, step)
    if (i >= 3 * a.K) return;
    const int ch = i / a.K, depth = i - ch * a.K;
    unsigned long long above = 0;
    for (int v = depth + 1; v <= a.K; ++v) above += a.hist[ch * kHistRow + v];
    // streams 1 + 2i and 2 + 2i <= 6K = n_streams - 1
    if (a.streams[1 + 2 * i].expect != above || a.streams[2 + 2 * i].expect != above) {
        a.hist[kSizesDiffer] = 1u;
        atomicOr(a.error, 1);
    }
}

__global__ __launch_bounds__(256) void mp_parse_void_kernel(const ParseArgs a)
{
    if (!a.hist[kSizesDiffer]) return;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < a.n_counts; i += (unsigned long long)gridDim.x * 256)
        a.counts[i] = 0;
}

// a view: the lengths cut to its steps (launch_clamp_lengths); i < n_counts, the host's size of `counts`
__global__ __launch_bounds__(256) void mp_parse_clamp_kernel(const ParseArgs a, unsigned steps)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < a.n_counts; i += (unsigned long long)gridDim.x * 256) {
        const unsigned c = a.counts[i];
        if (c > steps) a.counts[i] = (uint16_t)steps;
    }
}

namespace {
bool parse_args_ok(const ParseArgs& a) {
    return !(a.n_streams < 2 || a.n_streams > 6 * kMaxDeviceK + 1 || a.K < 1 || a.K > kMaxDeviceK || a.interval < 1 || a.n_counts < 3);
}
// groups [0, lengths_groups) of the grid are the lengths stream's when it is launched alone
int launch_parse_front(const ParseArgs& a, unsigned groups, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(a.hist, 0, sizeof(unsigned) * (kSizesDiffer + 1), s);
    if (e != hipSuccess) return (int)e;
    if (groups) hipLaunchKernelGGL(mp_parse_kernel<false>, dim3(groups), dim3(64), 0, s, a);
    const unsigned long long want = (a.n_counts + 255) / 256;
    const unsigned blocks = (unsigned)(want < 1024 ? want : 1024);
    hipLaunchKernelGGL(mp_parse_hist_kernel, dim3(blocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(mp_parse_verify_kernel, dim3(1), dim3(128), 0, s, a);
    hipLaunchKernelGGL(mp_parse_void_kernel, dim3(blocks), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}
}  // namespace

int launch_parse(const ParseArgs& a, void* stream_)
{
    if (!parse_args_ok(a)) return (int)hipErrorInvalidValue;
    return launch_parse_front(a, a.n_groups, static_cast<hipStream_t>(stream_));
}

int launch_parse_lengths(const ParseArgs& a, void* stream_)
{
    if (!parse_args_ok(a) || a.group_first > a.n_groups) return (int)hipErrorInvalidValue;
    return launch_parse_front(a, a.group_first, static_cast<hipStream_t>(stream_));
}

int launch_clamp_lengths(const ParseArgs& a, int steps, void* stream_)
{
    if (!parse_args_ok(a) || steps < 1 || steps > a.K) return (int)hipErrorInvalidValue;
    const unsigned long long want = (a.n_counts + 255) / 256;
    const unsigned blocks = (unsigned)(want < 1024 ? want : 1024);
    hipLaunchKernelGGL(mp_parse_clamp_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream_), a, (unsigned)steps);
    return (int)hipGetLastError();
}

int launch_parse_window(const ParseArgs& a, void* stream_)
{
    if (!parse_args_ok(a) || a.group_first > a.n_groups || !a.window) return (int)hipErrorInvalidValue;
    if (a.n_groups > a.group_first)
        hipLaunchKernelGGL(mp_parse_kernel<true>, dim3(a.n_groups - a.group_first), dim3(64), 0, static_cast<hipStream_t>(stream_), a);
    return (int)hipGetLastError();
}

}  // namespace mpc
