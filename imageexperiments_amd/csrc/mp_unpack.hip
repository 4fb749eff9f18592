// mp_unpack.hip -- product: the decoder's per-symbol work on the device, in front of mp_stream_gather_kernel: the mirror of what
// mp_entropy.hip (run lengths) and mp_streams.hip (dc) do in the encode direction.
//
// Input: the 6K streams of a container as the host's serial parse leaves them (entropy codes undone, nothing else): run-length
// packed where the container's flag says so (Huffman.cpp:246-279), the three step-0 coefficient streams difference coded
// (CompressedImage.cpp:428-446).  Output: the streams as launch_stream_gather reads them.
//
//   map     per block of 2048 coded symbols of a packed stream: runLengthDecode (Huffman.cpp:281-307) is a three-state machine
//           (fresh -> value; value -> count if the symbol repeats the one before it, else value; count -> emit, fresh).  What a
//           symbol is depends on its whole prefix, but only through that state: the block's 3 -> 3 state map and the symbols it
//           emits from each entry state, by a scan whose operator is map composition
//   carry   one wave per stream composes the blocks' maps in order: every block's entry state and first output position, and
//           the stream's total, compared with what the lengths stream allows BEFORE anything is written
//   fill    the same scan again from the known entry state gives every symbol's output position; the block's output range is
//           then written position by position (binary search over the 2048 start positions in LDS), so a run of 0x8000 copies
//           is spread over all lanes; streams that are not packed are copied
//   dc sum / dc scan   inclusive sums of zigzagDecode over the three step-0 coefficient streams (CompressedImage.cpp:690-705),
//           in place, wrapping 32-bit sums truncated to 16 bits
//
// The input is untrusted.  The stream table (UnpackStream) is built by the host from sizes it has checked: coded_off + coded_len
// lies inside `coded`, out_off + expect inside `symbols`, and a stream has exactly ceil(coded_len / 2048) blocks.  Every index
// below is bounded by those four numbers, never by a value read from the symbols; the comment at each access says how.
// Global memory is touched in aligned 4-byte words through LDS (two symbols a word); both buffers hold an even number of symbols.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mp_device.h"

namespace mpc {

namespace {
constexpr int kThreads = 256;
constexpr int kPerThread = kUnpackBlock / kThreads;        // 8 consecutive symbols a thread
constexpr int kWaves = kThreads / 64;
constexpr unsigned kIdentityMap = 0u | (1u << 2) | (2u << 4);
constexpr unsigned kMapRepeat = 1u | (2u << 2) | (0u << 4);    // fresh -> value, value -> count, count -> fresh
constexpr unsigned kMapOther = 1u | (1u << 2) | (0u << 4);     // fresh -> value, value -> value, count -> fresh

// A piece of a packed stream: where each entry state (0 fresh, 1 value, 2 count) leaves the machine, two bits each, and how many
// symbols the piece emits from that entry state.  T = unsigned inside a block (at most 2048 x 65535), 64 bits across blocks.
template <class T>
struct Piece {
    unsigned map;
    T out0, out1, out2;             // named members, not an array: a state-indexed array would live in scratch
};
__device__ __forceinline__ unsigned leave(unsigned map, unsigned state) { return (map >> (2u * state)) & 3u; }
template <class T>
__device__ __forceinline__ T emitted(const Piece<T>& p, unsigned state) {
    const T o0 = p.out0, o1 = p.out1, o2 = p.out2;             // values first: a choice between the members' addresses would put the piece in scratch
    return state == 0 ? o0 : state == 1 ? o1 : o2;
}
template <class T>
__device__ __forceinline__ Piece<T> identity_piece() { return Piece<T>{kIdentityMap, 0, 0, 0}; }
// `a` then `b`
template <class T>
__device__ __forceinline__ Piece<T> compose(const Piece<T>& a, const Piece<T>& b) {
    const unsigned m0 = leave(a.map, 0), m1 = leave(a.map, 1), m2 = leave(a.map, 2);
    Piece<T> r;
    r.map = leave(b.map, m0) | (leave(b.map, m1) << 2) | (leave(b.map, m2) << 4);
    r.out0 = a.out0 + emitted(b, m0);
    r.out1 = a.out1 + emitted(b, m1);
    r.out2 = a.out2 + emitted(b, m2);
    return r;
}
__device__ __forceinline__ unsigned long long shfl_up64(unsigned long long v, int d) {
    const unsigned lo = __shfl_up((unsigned)v, d), hi = __shfl_up((unsigned)(v >> 32), d);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int lane) {
    const unsigned lo = __shfl((unsigned)v, lane), hi = __shfl((unsigned)(v >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ Piece<unsigned> shfl_up_piece(const Piece<unsigned>& p, int d) {
    Piece<unsigned> r;
    r.map = __shfl_up(p.map, d);
    r.out0 = __shfl_up(p.out0, d);
    r.out1 = __shfl_up(p.out1, d);
    r.out2 = __shfl_up(p.out2, d);
    return r;
}
__device__ __forceinline__ Piece<unsigned long long> shfl_up_piece(const Piece<unsigned long long>& p, int d) {
    Piece<unsigned long long> r;
    r.map = __shfl_up(p.map, d);
    r.out0 = shfl_up64(p.out0, d);
    r.out1 = shfl_up64(p.out1, d);
    r.out2 = shfl_up64(p.out2, d);
    return r;
}
// inclusive scan over the wave's lanes in lane order; *before: the composition of the lanes in front of this one
template <class T>
__device__ __forceinline__ Piece<T> wave_scan(Piece<T> mine, int lane, Piece<T>* before) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const Piece<T> o = shfl_up_piece(mine, d);
        if (lane >= d) mine = compose(o, mine);
    }
    const Piece<T> o = shfl_up_piece(mine, 1);
    *before = lane ? o : identity_piece<T>();
    return mine;
}

// the stream block `b` belongs to: the last one whose first block is not behind b (streams without symbols have no blocks).
// streams[n_streams].blk_begin = n_blocks > b, so the result is < n_streams
__device__ __forceinline__ int stream_of_block(const UnpackArgs& a, unsigned b) {
    int lo = 0, hi = a.n_streams;                                 // invariant: streams[lo].blk_begin <= b < streams[hi].blk_begin
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.streams[mid].blk_begin <= b) lo = mid; else hi = mid;
    }
    return lo;
}

// symbols [begin, begin + n) of `buf` -> lds[0, n), read as aligned words.  The caller guarantees begin + n <= cap, and cap (the
// symbols the buffer holds) is even: the last word read, (begin + n - 1) / 2, ends at or before symbol cap.
__device__ __forceinline__ void load_span(const uint16_t* buf, unsigned long long begin, unsigned n, uint16_t* lds) {
    const unsigned long long end = begin + n, w0 = begin >> 1, w1 = (end + 1) >> 1;
    for (unsigned long long w = w0 + threadIdx.x; w < w1; w += kThreads) {
        const uint32_t v = reinterpret_cast<const uint32_t*>(buf)[w];
        const unsigned long long e = 2 * w;
        if (e >= begin) lds[e - begin] = (uint16_t)v;             // e < end: w <= w1 - 1 = (end - 1) / 2
        if (e + 1 >= begin && e + 1 < end) lds[e + 1 - begin] = (uint16_t)(v >> 16);
    }
}
// lds[0, n) -> symbols [begin, begin + n) of `buf`: whole words where both halves are inside the span, single symbols at its ends
// (the neighbouring spans belong to other workgroups).  The caller guarantees begin + n <= the buffer's symbols.
__device__ __forceinline__ void store_span(uint16_t* buf, unsigned long long begin, unsigned n, const uint16_t* lds) {
    const unsigned long long end = begin + n, w0 = begin >> 1, w1 = (end + 1) >> 1;
    for (unsigned long long w = w0 + threadIdx.x; w < w1; w += kThreads) {
        const unsigned long long e = 2 * w;
        const bool lo = e >= begin && e < end, hi = e + 1 >= begin && e + 1 < end;
        if (lo && hi) reinterpret_cast<uint32_t*>(buf)[w] = (uint32_t)lds[e - begin] | ((uint32_t)lds[e + 1 - begin] << 16);
        else if (lo) buf[e] = lds[e - begin];
        else if (hi) buf[e + 1] = lds[e + 1 - begin];
    }
}

// What a block of a packed stream has in LDS: sym[0] = the symbol in front of the block (unused at a stream's start),
// sym[1 + j] = its j-th symbol
struct BlockSpan {
    unsigned long long first;       // the block's first symbol in its stream
    unsigned n;                     // its symbols (1 .. 2048)
};
__device__ __forceinline__ BlockSpan load_block(const UnpackArgs& a, const UnpackStream& st, unsigned b, uint16_t* sym) {
    BlockSpan s;
    s.first = (unsigned long long)(b - st.blk_begin) * kUnpackBlock;          // < coded_len: the stream has ceil(coded_len / 2048) blocks
    const unsigned long long left = st.coded_len - s.first;
    s.n = left < (unsigned long long)kUnpackBlock ? (unsigned)left : (unsigned)kUnpackBlock;
    const unsigned halo = s.first ? 1u : 0u;
    // [coded_off + first - halo, coded_off + first + n) lies inside the stream's [coded_off, coded_off + coded_len), which the host
    // placed inside `coded`
    load_span(a.coded, st.coded_off + s.first - halo, s.n + halo, sym + 1 - halo);
    __syncthreads();
    return s;
}

// the thread's 8 symbols as one piece; sym as load_block leaves it
__device__ __forceinline__ Piece<unsigned> thread_piece(const BlockSpan& s, const uint16_t* sym) {
    Piece<unsigned> p = identity_piece<unsigned>();
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const unsigned j = threadIdx.x * kPerThread + k;
        if (j < s.n) {                                            // sym[j], sym[j + 1]: j + 1 <= n <= 2048
            const unsigned cur = sym[j + 1];
            const bool repeat = (s.first + j) != 0 && cur == sym[j];          // a stream's first symbol is always a value
            p = compose(p, Piece<unsigned>{repeat ? kMapRepeat : kMapOther, 1u, 1u, cur});
        }
    }
    return p;
}

// scan of the threads' pieces over the workgroup: returns what lies in front of this thread; *whole: the block's piece
__device__ __forceinline__ Piece<unsigned> block_scan(const Piece<unsigned>& mine, Piece<unsigned>* wave_piece /*[kWaves] LDS*/,
                                                      Piece<unsigned>* whole) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Piece<unsigned> before;
    const Piece<unsigned> incl = wave_scan(mine, lane, &before);
    if (lane == 63) wave_piece[wave] = incl;
    __syncthreads();
    Piece<unsigned> front = identity_piece<unsigned>(), all = identity_piece<unsigned>();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        if (w < wave) front = compose(front, wave_piece[w]);
        all = compose(all, wave_piece[w]);
    }
    *whole = all;
    return compose(front, before);
}
}  // namespace

__global__ __launch_bounds__(kThreads) void mp_unpack_map_kernel(const UnpackArgs a)
{
    __shared__ uint16_t sym[kUnpackBlock + 2];
    __shared__ Piece<unsigned> wave_piece[kWaves];
    const unsigned b = blockIdx.x;                                // < n_blocks (the grid)
    const UnpackStream& st = a.streams[stream_of_block(a, b)];
    if (!(st.flags & kUnpackPacked)) return;
    const BlockSpan s = load_block(a, st, b, sym);
    Piece<unsigned> whole;
    block_scan(thread_piece(s, sym), wave_piece, &whole);
    if (threadIdx.x == 0) reinterpret_cast<uint4*>(a.blk_piece)[b] = make_uint4(whole.map, whole.out0, whole.out1, whole.out2);
}

// one wave per stream
__global__ __launch_bounds__(64) void mp_unpack_carry_kernel(const UnpackArgs a)
{
    const int si = blockIdx.x, lane = threadIdx.x;                // si < n_streams (the grid)
    const UnpackStream& st = a.streams[si];
    const unsigned nb = a.streams[si + 1].blk_begin - st.blk_begin;
    bool ok;
    if (!(st.flags & kUnpackPacked)) {
        ok = st.coded_len == st.expect;
    } else {
        unsigned state = 0;                                       // fresh
        unsigned long long run = 0;
        for (unsigned base = 0; base < nb; base += 64) {
            const unsigned k = base + lane;
            Piece<unsigned long long> mine = identity_piece<unsigned long long>();
            if (k < nb) {                                         // blk_begin + k < the next stream's blk_begin <= n_blocks
                const uint4 v = reinterpret_cast<const uint4*>(a.blk_piece)[st.blk_begin + k];
                mine = Piece<unsigned long long>{v.x, v.y, v.z, v.w};
            }
            Piece<unsigned long long> before;
            const Piece<unsigned long long> incl = wave_scan(mine, lane, &before);
            if (k < nb) {
                a.blk_entry[st.blk_begin + k] = leave(before.map, state);
                a.blk_out[st.blk_begin + k] = run + emitted(before, state);
            }
            const unsigned all_map = __shfl(incl.map, 63);
            const unsigned long long all_out = shfl64(emitted(incl, state), 63);
            run += all_out;                                       // at most 2^32 blocks x 2048 x 65535 < 2^64
            state = leave(all_map, state);
        }
        ok = run == st.expect;                                    // a count left dangling at the end (state 2) is dropped, as on the host
    }
    if (lane == 0) {
        a.stream_ok[si] = ok ? 1u : 0u;
        if (!ok) atomicOr(a.error, 1);
    }
}

// kWindow (launch_unpack_window): of a stream that is copied and not summed -- not packed, no step-0 coefficient stream -- only the
// blocks that hold the window's positions [r0, r1) are copied: coded and expanded positions are the same there, and the rest of
// the stream may never have been parsed.  (r0, r1) only choose among the blocks; what a block reads and writes is bounded as before.
template <bool kWindow>
__global__ __launch_bounds__(kThreads) void mp_unpack_fill_kernel(const UnpackArgs a)
{
    __shared__ uint16_t sym[kUnpackBlock + 2];
    __shared__ uint16_t value[kUnpackBlock];
    __shared__ unsigned start[kUnpackBlock];
    __shared__ Piece<unsigned> wave_piece[kWaves];
    const unsigned b = blockIdx.x;                                // < n_blocks (the grid)
    const int si = stream_of_block(a, b);
    const UnpackStream& st = a.streams[si];
    if (!a.stream_ok[si]) return;                                 // nothing is written for a stream whose size is not the expected one
    if (kWindow && !(st.flags & kUnpackPacked) && si != a.dc_stream[0] && si != a.dc_stream[1] && si != a.dc_stream[2]) {
        const WindowStream win = a.window[si];                    // si < n_streams
        const unsigned long long first = (unsigned long long)(b - st.blk_begin) * kUnpackBlock;
        if (first + kUnpackBlock <= win.r0 || first >= win.r1) return;       // the whole workgroup
    }
    const BlockSpan s = load_block(a, st, b, sym);
    if (!(st.flags & kUnpackPacked)) {
        // stream_ok: coded_len == expect, so first + n <= expect and the span ends inside the stream's [out_off, out_off + expect)
        store_span(a.symbols, st.out_off + s.first, s.n, sym + 1);
        return;
    }
    Piece<unsigned> whole;
    const Piece<unsigned> front = block_scan(thread_piece(s, sym), wave_piece, &whole);
    const unsigned entry = a.blk_entry[b];
    unsigned state = leave(front.map, entry), at = emitted(front, entry);
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const unsigned j = threadIdx.x * kPerThread + k;          // < 2048: start[], value[]
        start[j] = at;                                            // behind the block's last symbol: the block's total
        if (j < s.n) {
            const unsigned cur = sym[j + 1], prev = sym[j];
            if (state == 2) {
                value[j] = (uint16_t)prev;
                at += cur;
                state = 0;
            } else {
                value[j] = (uint16_t)cur;
                at += 1;
                state = (state == 1 && (s.first + j) != 0 && cur == prev) ? 2u : 1u;
            }
        }
    }
    __syncthreads();
    // The block's output [blk_out, blk_out + total) in its stream.  stream_ok: the blocks' totals add up to exactly `expect`, so
    // this range ends at or before `expect` and every position written lies inside the stream's [out_off, out_off + expect).
    const unsigned total = emitted(whole, entry);
    const unsigned long long begin = st.out_off + a.blk_out[b], end = begin + total;
    for (unsigned long long w = (begin >> 1) + threadIdx.x; w < ((end + 1) >> 1); w += kThreads) {
        uint16_t got[2] = {0, 0};
        bool in[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned long long e = 2 * w + h;
            in[h] = e >= begin && e < end;
            if (in[h]) {
                const unsigned p = (unsigned)(e - begin);         // < total
                unsigned j = 0;                                   // the last symbol whose output starts at or before p: start[0] = 0 <= p
#pragma unroll
                for (unsigned step = kUnpackBlock / 2; step; step >>= 1)
                    if (start[j + step] <= p) j += step;          // j + step <= 1024 + 512 + ... + 1 = 2047
                got[h] = value[j];
            }
        }
        if (in[0] && in[1]) reinterpret_cast<uint32_t*>(a.symbols)[w] = (uint32_t)got[0] | ((uint32_t)got[1] << 16);
        else if (in[0]) a.symbols[2 * w] = got[0];
        else if (in[1]) a.symbols[2 * w + 1] = got[1];
    }
}

namespace {
__device__ __forceinline__ int32_t zigzag_decode_dev(uint32_t x) { return (int32_t)((x >> 1) ^ (0u - (x & 1u))); }   // BitBuffer.h:117

// the dc block's stream (0..2), its first symbol in that stream and its symbols
__device__ __forceinline__ int dc_block(const UnpackArgs& a, unsigned d, unsigned long long* first, unsigned* n) {
    const int which = d >= a.dc_blk_begin[2] ? 2 : d >= a.dc_blk_begin[1] ? 1 : 0;
    const unsigned long long expect = a.streams[a.dc_stream[which]].expect;
    *first = (unsigned long long)(d - a.dc_blk_begin[which]) * kUnpackBlock;  // < expect: the stream has ceil(expect / 2048) dc blocks
    const unsigned long long left = expect - *first;
    *n = left < (unsigned long long)kUnpackBlock ? (unsigned)left : (unsigned)kUnpackBlock;
    return which;
}
__device__ __forceinline__ unsigned block_sum(unsigned v, unsigned* wave_sum /*[kWaves] LDS*/) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    __syncthreads();                                              // wave_sum of an earlier use is no longer read
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) all += wave_sum[w];
    return all;
}
}  // namespace

// sum of zigzagDecode over each 2048-symbol block of the expanded step-0 coefficient streams
__global__ __launch_bounds__(kThreads) void mp_unpack_dc_sum_kernel(const UnpackArgs a)
{
    __shared__ uint16_t sym[kUnpackBlock];
    __shared__ unsigned wave_sum[kWaves];
    const unsigned d = blockIdx.x;                                // < dc_blk_begin[3] (the grid)
    unsigned long long first;
    unsigned n;
    const int which = dc_block(a, d, &first, &n);
    const UnpackStream& st = a.streams[a.dc_stream[which]];
    if (!a.stream_ok[a.dc_stream[which]]) return;
    load_span(a.symbols, st.out_off + first, n, sym);             // first + n <= expect: inside the stream's output
    __syncthreads();
    unsigned acc = 0;
    for (unsigned j = threadIdx.x; j < n; j += kThreads) acc += (unsigned)zigzag_decode_dev(sym[j]);
    const unsigned all = block_sum(acc, wave_sum);
    if (threadIdx.x == 0) a.dc_part[d] = all;
}

__global__ __launch_bounds__(kThreads) void mp_unpack_dc_scan_kernel(const UnpackArgs a)
{
    __shared__ uint16_t sym[kUnpackBlock];
    __shared__ unsigned wave_sum[kWaves];
    __shared__ unsigned wave_incl[kWaves];
    const unsigned d = blockIdx.x;                                // < dc_blk_begin[3] (the grid)
    unsigned long long first;
    unsigned n;
    const int which = dc_block(a, d, &first, &n);
    const UnpackStream& st = a.streams[a.dc_stream[which]];
    if (!a.stream_ok[a.dc_stream[which]]) return;
    unsigned carry = 0;                                           // the blocks of this stream in front of d: dc_blk_begin[which] <= k < d
    for (unsigned k = a.dc_blk_begin[which] + threadIdx.x; k < d; k += kThreads) carry += a.dc_part[k];
    carry = block_sum(carry, wave_sum);
    load_span(a.symbols, st.out_off + first, n, sym);
    __syncthreads();
    unsigned v[kPerThread], mine = 0;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const unsigned j = threadIdx.x * kPerThread + k;          // < 2048
        mine += j < n ? (unsigned)zigzag_decode_dev(sym[j]) : 0u;
        v[k] = mine;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned incl = mine;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned o = __shfl_up(incl, s);
        if (lane >= s) incl += o;
    }
    if (lane == 63) wave_incl[wave] = incl;
    __syncthreads();                                              // also: every thread has read its sym[] before they are overwritten
    unsigned front = carry + incl - mine;
#pragma unroll
    for (int w = 0; w < kWaves; ++w)
        if (w < wave) front += wave_incl[w];
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const unsigned j = threadIdx.x * kPerThread + k;
        if (j < n) sym[j] = (uint16_t)(front + v[k]);             // the reference's low 16 bits of the running sum
    }
    __syncthreads();
    store_span(a.symbols, st.out_off + first, n, sym);            // this block's own symbols only
}


// ------------------------------------------------------------------------------------------------
// The window of a version-2 index (launch_unpack_window_cut).  A stream with kSpanCut -- run-length packed, or a step-0 coefficient
// stream -- had only its coded symbols [s0, s1) parsed; the rest of its part of `coded` was never written.  The machine is entered
// at s0 in state0 at output position out0, the symbol in front of s0 is prev0 (never the memory in front, which nobody parsed), and
// behind s1 - 1 the position, the state and that symbol must be the index's exit values before anything is written.  Blocks stay
// the stream's own blocks of 2048 coded symbols, so s0 is in general inside a block: symbols of a block outside [s0, s1) are
// identity pieces, blocks wholly outside leave at once.  Every bound is the host's: s0 <= s1 <= coded_len and out0 <= out1 <= expect
// are cut here once more (mp_window_rank_kernel<true> has cut them already); no symbol's value bounds anything.
// ------------------------------------------------------------------------------------------------
namespace {
struct CutRange {
    unsigned long long s0, s1;      // s0 <= s1 <= coded_len
    unsigned long long out0, out1;  // out0 <= out1 <= expect
    bool cut, check;
};
__device__ __forceinline__ CutRange cut_range(const WindowSpan& sp, const UnpackStream& st) {
    CutRange c;
    c.cut = (sp.flags & kSpanCut) != 0u;
    c.check = c.cut && (sp.flags & kSpanCheck) != 0u;
    c.s1 = !c.cut ? st.coded_len : sp.s1 < st.coded_len ? sp.s1 : st.coded_len;
    c.s0 = !c.cut ? 0ull : sp.s0 < c.s1 ? sp.s0 : c.s1;
    c.out1 = !c.cut ? st.expect : sp.out1 < st.expect ? sp.out1 : st.expect;
    c.out0 = !c.cut ? 0ull : sp.out0 < c.out1 ? sp.out0 : c.out1;
    return c;
}
// the block holds none of [s0, s1): the whole workgroup
__device__ __forceinline__ bool block_outside(unsigned long long first, unsigned long long s0, unsigned long long s1) {
    return s0 >= s1 || first + kUnpackBlock <= s0 || first >= s1;
}
// thread_piece with the symbols outside [s0, s1) as identity pieces and prev0 in front of s0
__device__ __forceinline__ Piece<unsigned> thread_piece_cut(const BlockSpan& s, const uint16_t* sym, unsigned long long s0, unsigned long long s1,
                                                            unsigned prev0) {
    Piece<unsigned> p = identity_piece<unsigned>();
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const unsigned j = threadIdx.x * kPerThread + k;
        const unsigned long long pos = s.first + j;
        if (j < s.n && pos >= s0 && pos < s1) {                   // sym[j], sym[j + 1]: j + 1 <= n <= 2048
            const unsigned cur = sym[j + 1];
            const unsigned before = pos == s0 ? prev0 : sym[j];  // pos > s0: symbol pos - 1 was parsed
            const bool repeat = pos != 0 && cur == before;
            p = compose(p, Piece<unsigned>{repeat ? kMapRepeat : kMapOther, 1u, 1u, cur});
        }
    }
    return p;
}
}  // namespace

__global__ __launch_bounds__(kThreads) void mp_unpack_window_map_kernel(const UnpackWindowArgs w)
{
    __shared__ uint16_t sym[kUnpackBlock + 2];
    __shared__ Piece<unsigned> wave_piece[kWaves];
    const UnpackArgs& a = w.a;
    const unsigned b = blockIdx.x;                                // < n_blocks (the grid)
    const int si = stream_of_block(a, b);
    const UnpackStream& st = a.streams[si];
    if (!(st.flags & kUnpackPacked)) return;
    const WindowSpan sp = w.span[si];                             // si < n_streams
    const CutRange c = cut_range(sp, st);
    if (block_outside((unsigned long long)(b - st.blk_begin) * kUnpackBlock, c.s0, c.s1)) return;
    const BlockSpan s = load_block(a, st, b, sym);                // inside the stream's own part of `coded`, parsed or not
    Piece<unsigned> whole;
    block_scan(thread_piece_cut(s, sym, c.s0, c.s1, sp.prev0), wave_piece, &whole);
    if (threadIdx.x == 0) reinterpret_cast<uint4*>(a.blk_piece)[b] = make_uint4(whole.map, whole.out0, whole.out1, whole.out2);
}

// one wave per stream: the blocks that hold [s0, s1) composed from (state0, out0), and the exit checks
__global__ __launch_bounds__(64) void mp_unpack_window_carry_kernel(const UnpackWindowArgs w)
{
    const UnpackArgs& a = w.a;
    const int si = blockIdx.x, lane = threadIdx.x;                // si < n_streams (the grid)
    const UnpackStream& st = a.streams[si];
    const unsigned nb = a.streams[si + 1].blk_begin - st.blk_begin;
    const WindowSpan sp = w.span[si];
    const CutRange c = cut_range(sp, st);
    bool ok;
    if (!(st.flags & kUnpackPacked)) {
        ok = st.coded_len == st.expect;
    } else if (c.s0 >= c.s1) {
        ok = c.cut || st.expect == 0;                             // nothing of the stream was parsed, nothing of it is written
    } else {
        unsigned state = c.cut ? (sp.state0 < 2u ? sp.state0 : 2u) : 0u;
        unsigned long long run = c.out0;
        // blocks [k0, k1) hold [s0, s1); k1 <= nb: s1 <= coded_len and the stream has ceil(coded_len / 2048) blocks
        const unsigned long long k0 = c.s0 / kUnpackBlock, k1 = (c.s1 + kUnpackBlock - 1) / kUnpackBlock;
        for (unsigned long long base = k0; base < k1 && base < nb; base += 64) {
            const unsigned long long k = base + lane;
            const bool mine_in = k < k1 && k < nb;
            Piece<unsigned long long> mine = identity_piece<unsigned long long>();
            if (mine_in) {                                        // blk_begin + k < the next stream's blk_begin <= n_blocks
                const uint4 v = reinterpret_cast<const uint4*>(a.blk_piece)[st.blk_begin + k];
                mine = Piece<unsigned long long>{v.x, v.y, v.z, v.w};
            }
            Piece<unsigned long long> before;
            const Piece<unsigned long long> incl = wave_scan(mine, lane, &before);
            if (mine_in) {
                a.blk_entry[st.blk_begin + k] = leave(before.map, state);
                a.blk_out[st.blk_begin + k] = run + emitted(before, state);
            }
            const unsigned all_map = __shfl(incl.map, 63);
            const unsigned long long all_out = shfl64(emitted(incl, state), 63);
            run += all_out;
            state = leave(all_map, state);
        }
        // the fill writes [out0, run) of the stream: run == out1 <= expect, decided here, before it writes
        ok = run == c.out1;
        if (c.check) {
            // coded_off + s1 - 1: s0 < s1 <= coded_len, the last symbol that was parsed
            const unsigned last = a.coded[st.coded_off + c.s1 - 1];
            ok = ok && state == sp.state1 && last == sp.prev1;
        }                                                         // else the stream's end: a count left dangling is dropped, as on the host
    }
    if (lane == 0) {
        a.stream_ok[si] = ok ? 1u : 0u;
        if (!ok) atomicOr(a.error, 1);
    }
}

__global__ __launch_bounds__(kThreads) void mp_unpack_window_fill_kernel(const UnpackWindowArgs w)
{
    __shared__ uint16_t sym[kUnpackBlock + 2];
    __shared__ uint16_t value[kUnpackBlock];
    __shared__ unsigned start[kUnpackBlock];
    __shared__ Piece<unsigned> wave_piece[kWaves];
    const UnpackArgs& a = w.a;
    const unsigned b = blockIdx.x;                                // < n_blocks (the grid)
    const int si = stream_of_block(a, b);
    const UnpackStream& st = a.streams[si];
    if (!a.stream_ok[si]) return;
    const WindowSpan sp = w.span[si];                             // si < n_streams
    const CutRange c = cut_range(sp, st);
    const unsigned long long first = (unsigned long long)(b - st.blk_begin) * kUnpackBlock;
    if (!(st.flags & kUnpackPacked)) {
        // coded and expanded positions are the same.  A step-0 coefficient stream: what was parsed, [s0, s1); any other stream: the
        // blocks that hold its window [r0, r1), as mp_unpack_fill_kernel<true> does
        unsigned long long lo = 0, hi = st.coded_len;
        if (c.cut) {
            if (block_outside(first, c.s0, c.s1)) return;         // the whole workgroup
            lo = c.s0;
            hi = c.s1;
        } else if (si != a.dc_stream[0] && si != a.dc_stream[1] && si != a.dc_stream[2]) {
            const WindowStream win = a.window[si];
            if (first + kUnpackBlock <= win.r0 || first >= win.r1) return;
        }
        const BlockSpan s = load_block(a, st, b, sym);
        const unsigned long long from = s.first > lo ? s.first : lo, to = s.first + s.n < hi ? s.first + s.n : hi;
        // stream_ok: coded_len == expect, so [from, to) inside the block's [first, first + n) ends inside [out_off, out_off + expect)
        if (from < to) store_span(a.symbols, st.out_off + from, (unsigned)(to - from), sym + 1 + (unsigned)(from - s.first));
        return;
    }
    if (block_outside(first, c.s0, c.s1)) return;                 // the whole workgroup
    const BlockSpan s = load_block(a, st, b, sym);
    Piece<unsigned> whole;
    const Piece<unsigned> front = block_scan(thread_piece_cut(s, sym, c.s0, c.s1, sp.prev0), wave_piece, &whole);
    const unsigned entry = a.blk_entry[b];
    unsigned state = leave(front.map, entry), at = emitted(front, entry);
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const unsigned j = threadIdx.x * kPerThread + k;          // < 2048: start[], value[]
        const unsigned long long pos = s.first + j;
        start[j] = at;                                            // a symbol outside [s0, s1) emits nothing: the next one's start
        value[j] = 0;
        if (j < s.n && pos >= c.s0 && pos < c.s1) {
            const unsigned cur = sym[j + 1], prev = pos == c.s0 ? sp.prev0 : sym[j];
            if (state == 2) {
                value[j] = (uint16_t)prev;
                at += cur;
                state = 0;
            } else {
                value[j] = (uint16_t)cur;
                at += 1;
                state = (state == 1 && pos != 0 && cur == prev) ? 2u : 1u;
            }
        }
    }
    __syncthreads();
    // The block's output [blk_out, blk_out + total) in its stream.  stream_ok: the blocks' totals lead from out0 to exactly
    // out1 <= expect, so every position written lies inside [out0, out1) of the stream's [out_off, out_off + expect).
    const unsigned total = emitted(whole, entry);
    const unsigned long long begin = st.out_off + a.blk_out[b], end = begin + total;
    for (unsigned long long wd = (begin >> 1) + threadIdx.x; wd < ((end + 1) >> 1); wd += kThreads) {
        uint16_t got[2] = {0, 0};
        bool in[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned long long e = 2 * wd + h;
            in[h] = e >= begin && e < end;
            if (in[h]) {
                const unsigned p = (unsigned)(e - begin);         // < total
                unsigned j = 0;                                   // the last symbol whose output starts at or before p: start[0] = 0 <= p
#pragma unroll
                for (unsigned step = kUnpackBlock / 2; step; step >>= 1)
                    if (start[j + step] <= p) j += step;          // j + step <= 2047
                got[h] = value[j];
            }
        }
        if (in[0] && in[1]) reinterpret_cast<uint32_t*>(a.symbols)[wd] = (uint32_t)got[0] | ((uint32_t)got[1] << 16);
        else if (in[0]) a.symbols[2 * wd] = got[0];
        else if (in[1]) a.symbols[2 * wd + 1] = got[1];
    }
}

// The DC sums over [out0, out1) of the expanded stream alone: the blocks of 2048 expanded symbols that hold it, positions in front
// of out0 contributing nothing, the carry seeded with dc0, and the sum behind out1 - 1 held to dc1 through the error word
__global__ __launch_bounds__(kThreads) void mp_unpack_window_dc_sum_kernel(const UnpackWindowArgs w)
{
    __shared__ uint16_t sym[kUnpackBlock];
    __shared__ unsigned wave_sum[kWaves];
    const UnpackArgs& a = w.a;
    const unsigned d = blockIdx.x;                                // < dc_blk_begin[3] (the grid)
    unsigned long long first;
    unsigned n;
    const int which = dc_block(a, d, &first, &n);
    const int si = a.dc_stream[which];
    const UnpackStream& st = a.streams[si];
    if (!a.stream_ok[si]) return;
    const CutRange c = cut_range(w.span[si], st);
    if (block_outside(first, c.out0, c.out1)) return;             // the whole workgroup
    load_span(a.symbols, st.out_off + first, n, sym);             // first + n <= expect: inside the stream's output
    __syncthreads();
    unsigned acc = 0;
    for (unsigned j = threadIdx.x; j < n; j += kThreads)
        if (first + j >= c.out0 && first + j < c.out1) acc += (unsigned)zigzag_decode_dev(sym[j]);      // what the fill wrote
    const unsigned all = block_sum(acc, wave_sum);
    if (threadIdx.x == 0) a.dc_part[d] = all;
}

__global__ __launch_bounds__(kThreads) void mp_unpack_window_dc_scan_kernel(const UnpackWindowArgs w)
{
    __shared__ uint16_t sym[kUnpackBlock];
    __shared__ unsigned wave_sum[kWaves];
    __shared__ unsigned wave_incl[kWaves];
    const UnpackArgs& a = w.a;
    const unsigned d = blockIdx.x;                                // < dc_blk_begin[3] (the grid)
    unsigned long long first;
    unsigned n;
    const int which = dc_block(a, d, &first, &n);
    const int si = a.dc_stream[which];
    const UnpackStream& st = a.streams[si];
    if (!a.stream_ok[si]) return;
    const WindowSpan sp = w.span[si];
    const CutRange c = cut_range(sp, st);
    if (block_outside(first, c.out0, c.out1)) return;             // the whole workgroup
    // the blocks of this stream from the one that holds out0 up to d: dc_blk_begin[which] <= k < d, all of them written by the sum kernel
    unsigned carry = 0;
    for (unsigned long long k = a.dc_blk_begin[which] + c.out0 / kUnpackBlock + threadIdx.x; k < d; k += kThreads) carry += a.dc_part[k];
    carry = block_sum(carry, wave_sum) + (c.cut ? sp.dc0 : 0u);
    load_span(a.symbols, st.out_off + first, n, sym);
    __syncthreads();
    unsigned v[kPerThread], mine = 0;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const unsigned j = threadIdx.x * kPerThread + k;          // < 2048
        const bool in = j < n && first + j >= c.out0 && first + j < c.out1;
        mine += in ? (unsigned)zigzag_decode_dev(sym[j]) : 0u;
        v[k] = mine;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned incl = mine;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned o = __shfl_up(incl, s);
        if (lane >= s) incl += o;
    }
    if (lane == 63) wave_incl[wave] = incl;
    __syncthreads();                                              // also: every thread has read its sym[] before they are overwritten
    unsigned front = carry + incl - mine, all = carry;
#pragma unroll
    for (int wv = 0; wv < kWaves; ++wv) {
        if (wv < wave) front += wave_incl[wv];
        all += wave_incl[wv];
    }
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const unsigned j = threadIdx.x * kPerThread + k;
        if (j < n) sym[j] = (uint16_t)(front + v[k]);
    }
    __syncthreads();
    const unsigned long long from = first > c.out0 ? first : c.out0, to = first + n < c.out1 ? first + n : c.out1;
    if (from < to) store_span(a.symbols, st.out_off + from, (unsigned)(to - from), sym + (unsigned)(from - first));   // inside [out0, out1) and this block
    // the block that holds out1 - 1 has the sum behind it
    if (c.check && threadIdx.x == 0 && c.out1 <= first + n && (all & 0xFFFFu) != sp.dc1) atomicOr(a.error, 1);
}

namespace {
template <bool kWindow>
int launch_unpack_as(const UnpackArgs& a, void* stream_)
{
    hipStream_t s = static_cast<hipStream_t>(stream_);
    if (a.n_streams < 1 || a.n_streams > 6 * kMaxDeviceK || (kWindow && !a.window)) return (int)hipErrorInvalidValue;
    if (a.n_blocks) hipLaunchKernelGGL(mp_unpack_map_kernel, dim3(a.n_blocks), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(mp_unpack_carry_kernel, dim3((unsigned)a.n_streams), dim3(64), 0, s, a);
    if (a.n_blocks) hipLaunchKernelGGL(mp_unpack_fill_kernel<kWindow>, dim3(a.n_blocks), dim3(kThreads), 0, s, a);
    if (a.dc_blk_begin[3]) {
        hipLaunchKernelGGL(mp_unpack_dc_sum_kernel, dim3(a.dc_blk_begin[3]), dim3(kThreads), 0, s, a);
        hipLaunchKernelGGL(mp_unpack_dc_scan_kernel, dim3(a.dc_blk_begin[3]), dim3(kThreads), 0, s, a);
    }
    return (int)hipGetLastError();
}
}  // namespace

int launch_unpack(const UnpackArgs& a, void* stream) { return launch_unpack_as<false>(a, stream); }
int launch_unpack_window(const UnpackArgs& a, void* stream) { return launch_unpack_as<true>(a, stream); }

int launch_unpack_window_cut(const UnpackWindowArgs& w, void* stream_)
{
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const UnpackArgs& a = w.a;
    if (a.n_streams < 1 || a.n_streams > 6 * kMaxDeviceK || !a.window || !w.span) return (int)hipErrorInvalidValue;
    if (a.n_blocks) hipLaunchKernelGGL(mp_unpack_window_map_kernel, dim3(a.n_blocks), dim3(kThreads), 0, s, w);
    hipLaunchKernelGGL(mp_unpack_window_carry_kernel, dim3((unsigned)a.n_streams), dim3(64), 0, s, w);
    if (a.n_blocks) hipLaunchKernelGGL(mp_unpack_window_fill_kernel, dim3(a.n_blocks), dim3(kThreads), 0, s, w);
    if (a.dc_blk_begin[3]) {
        hipLaunchKernelGGL(mp_unpack_window_dc_sum_kernel, dim3(a.dc_blk_begin[3]), dim3(kThreads), 0, s, w);
        hipLaunchKernelGGL(mp_unpack_window_dc_scan_kernel, dim3(a.dc_blk_begin[3]), dim3(kThreads), 0, s, w);
    }
    return (int)hipGetLastError();
}

}  // namespace mpc
