// mp_streams.hip -- product: device-side stream assembly for the MI355X tile encoder.
//
// The container holds, besides `lengths`, 6K symbol streams: codes[2K*ch + 2i] = deltaId and [+1] = intCoeff of step i of
// channel ch for every tile with more than i atoms, tiles in the reference's visiting order (x outer, y inner:
// CompressedImage.cpp:535-572); the three step-0 coefficient streams are difference coded (:428-446).  The pursuit leaves
// records [tile][3][K] of which most are dead (97 MB for a 16 Mpixel K = 32 frame, 21 MB alive).  These kernels compact the
// live symbols stream by stream, in stream order, into ONE contiguous u16 buffer laid out in container order and apply the
// DC differencing, so that only the live symbols cross PCIe and every host coding job starts from a finished stream:
//   count    per block of 1024 tiles and channel: tiles with more than i atoms, for every i (from a histogram of the counts)
//   scan     exclusive scan of those over the blocks (one wave per stream pair); stream sizes
//   scatter  stream offsets from the sizes; rank of every live symbol inside its block by ballots, write deltaId / intCoeff to
//            their stream positions
//   dc       zig-zag difference of the three step-0 coefficient streams (CompressedImage.cpp:428-446)
// HBM-bound byte shuffling: reads are 16-byte vectors of whole records, writes are runs of consecutive u16.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mp_device.h"

namespace mpc {

namespace {
constexpr int kBlockTiles = 1024;               // tiles per workgroup (thread = tile)
constexpr int kWavesPerBlock = kBlockTiles / 64;
}  // namespace

__global__ __launch_bounds__(kBlockTiles) void mp_stream_count_kernel(const StreamArgs a)
{
    __shared__ unsigned hist[3][kMaxDeviceK + 2];
    for (int i = threadIdx.x; i < 3 * (kMaxDeviceK + 2); i += kBlockTiles) (&hist[0][0])[i] = 0;
    __syncthreads();
    const long long t = (long long)blockIdx.x * kBlockTiles + threadIdx.x;
    if (t < a.tiles) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int c = a.counts[t * 3 + ch];
            atomicAdd(&hist[ch][c < a.K ? c : a.K], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 3 * a.K) {
        const int ch = threadIdx.x / a.K, i = threadIdx.x - ch * a.K;
        unsigned live = 0;
        for (int c = i + 1; c <= a.K; ++c) live += hist[ch][c];
        a.block_live[((long long)blockIdx.x * 3 + ch) * a.K + i] = live;
    }
}

// one wave per (channel, step): exclusive scan of the live counts over the blocks, in place; the stream's size
__global__ __launch_bounds__(64) void mp_stream_scan_kernel(const StreamArgs a, int blocks)
{
    const int pair = blockIdx.x, ch = pair / a.K, i = pair - ch * a.K, lane = threadIdx.x;
    unsigned run = 0;
    for (int base = 0; base < blocks; base += 64) {
        const int b = base + lane;
        const long long at = ((long long)(b < blocks ? b : 0) * 3 + ch) * a.K + i;
        const unsigned n = b < blocks ? a.block_live[at] : 0u;
        unsigned incl = n;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (b < blocks) a.block_live[at] = run + incl - n;            // live count -> offset of the block in its stream
        run += __shfl(incl, 63);
    }
    if (lane == 0) a.sizes[pair] = run;
}

// the streams in container order: codes[2K*ch + 2i] = deltaId, [+1] = intCoeff, each sizes[ch*K + i] symbols
__device__ __forceinline__ void stream_layout(const StreamArgs& a, unsigned long long* off /*[6K + 1], LDS*/)
{
    if (threadIdx.x == 0) {
        unsigned long long at = 0;
        for (int p = 0; p < 3 * a.K; ++p) {
            const unsigned n = a.sizes[p];
            off[2 * p] = at;
            at += n;
            off[2 * p + 1] = at;
            at += n;
        }
        off[6 * a.K] = at;
    }
    __syncthreads();
}

__global__ __launch_bounds__(kBlockTiles) void mp_stream_scatter_kernel(const StreamArgs a)
{
    __shared__ unsigned wave_live[kWavesPerBlock][kMaxDeviceK];   // live tiles of the waves in front of this one, per step
    __shared__ unsigned block_at[3 * kMaxDeviceK];                // the block's first position in each stream
    __shared__ unsigned long long off[6 * kMaxDeviceK + 1];
    stream_layout(a, off);
    if (blockIdx.x == 0)                                          // for the kernels and copies that follow
        for (int s = threadIdx.x; s <= 6 * a.K; s += kBlockTiles) a.stream_off[s] = off[s];
    if ((int)threadIdx.x < 3 * a.K) block_at[threadIdx.x] = a.block_live[(long long)blockIdx.x * 3 * a.K + threadIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long t = (long long)blockIdx.x * kBlockTiles + threadIdx.x;
    const bool in = t < a.tiles;
    const unsigned long long below = (1ULL << lane) - 1ULL;
    for (int ch = 0; ch < 3; ++ch) {
        const int c = in ? min((int)a.counts[t * 3 + ch], a.K) : 0;
        // only the live part of the record is read: a lane asks for the 16-byte pieces that hold its first c steps (most
        // tile-channels stop after a few steps, and the dead steps are three quarters of the records' bytes)
        uint32_t rec[kMaxDeviceK];
        {
            const uint4* src = reinterpret_cast<const uint4*>(a.choices + ((in ? t : 0) * 3 + ch) * a.K);
#pragma unroll
            for (int v = 0; v < kMaxDeviceK / 4; ++v) {
                uint4 x = make_uint4(0, 0, 0, 0);
                if (4 * v < c && (a.K & 3) == 0) x = src[v];
                rec[4 * v] = x.x; rec[4 * v + 1] = x.y; rec[4 * v + 2] = x.z; rec[4 * v + 3] = x.w;
            }
            if ((a.K & 3) != 0) {                                // K not a multiple of 4: records are not 16-byte aligned
                const uint32_t* s1 = a.choices + ((in ? t : 0) * 3 + ch) * a.K;
#pragma unroll
                for (int i = 0; i < kMaxDeviceK; ++i) rec[i] = i < c ? s1[i] : 0u;
            }
        }
        __syncthreads();                                          // wave_live of the previous channel is no longer read
#pragma unroll
        for (int i = 0; i < kMaxDeviceK; ++i)
            if (i < a.K) {
                const unsigned long long live = __ballot(c > i);
                if (lane == 0) wave_live[wave][i] = (unsigned)__popcll(live);
            }
        __syncthreads();
        if ((int)threadIdx.x < a.K) {                             // counts -> exclusive prefix over the waves, once per step
            unsigned run = 0;
#pragma unroll
            for (int w = 0; w < kWavesPerBlock; ++w) {
                const unsigned n = wave_live[w][threadIdx.x];
                wave_live[w][threadIdx.x] = run;
                run += n;
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kMaxDeviceK; ++i)
            if (i < a.K) {
                const unsigned long long live = __ballot(c > i);
                if (!live) continue;
                if (c > i) {
                    const unsigned long long pos = (unsigned long long)block_at[ch * a.K + i] + wave_live[wave][i] + (unsigned)__popcll(live & below);
                    const unsigned long long od = off[2 * (ch * a.K + i)], oc = off[2 * (ch * a.K + i) + 1];
                    a.symbols[od + pos] = (uint16_t)(rec[i] & 0xFFFFu);
                    // step-0 coefficients go through the difference kernel: parked behind the end of all streams
                    uint16_t* coeff = i == 0 ? a.dc_tmp + (long long)ch * a.tiles : a.symbols + oc;
                    coeff[pos] = (uint16_t)(rec[i] >> 16);
                }
            }
    }
}

// The inverse of the scatter, for the decoder (CompressedImage.cpp:680-705 read the streams back into per-tile records): the same
// positions -- block offset + rank inside the block -- but the symbols are READ from the 6K streams (`symbols`, laid out as the
// scatter writes them; the step-0 coefficients already summed up by the host) and every tile's records written whole, dead steps
// as zeros.
// kWindow: a launch over the blocks that hold the tiles [t0, t1), the first of them block_first.  Every tile of those blocks still
// counts in the ballots (a position is a rank among ALL tiles in front), but only the window's tiles read symbols and write
// records: the streams outside the window were never parsed.
template <bool kWindow>
__global__ __launch_bounds__(kBlockTiles) void mp_stream_gather_kernel(const StreamArgs a, uint32_t* __restrict__ choices, unsigned block_first,
                                                                       long long t0, long long t1)
{
    __shared__ unsigned wave_live[kWavesPerBlock][kMaxDeviceK];
    __shared__ unsigned long long off[6 * kMaxDeviceK + 1];
    stream_layout(a, off);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long block = kWindow ? (long long)blockIdx.x + block_first : (long long)blockIdx.x;
    const long long t = block * kBlockTiles + threadIdx.x;
    const bool in = t < a.tiles;
    const bool wanted = kWindow ? in && t >= t0 && t < t1 : in;
    const unsigned long long below = (1ULL << lane) - 1ULL;
    for (int ch = 0; ch < 3; ++ch) {
        const int c = in ? (int)a.counts[t * 3 + ch] : 0;
        uint32_t rec[kMaxDeviceK];
        __syncthreads();                                          // wave_live of the previous channel is no longer read
#pragma unroll
        for (int i = 0; i < kMaxDeviceK; ++i)
            if (i < a.K) {
                const unsigned long long live = __ballot(c > i);
                if (lane == 0) wave_live[wave][i] = (unsigned)__popcll(live);
            }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kMaxDeviceK; ++i) {
            rec[i] = 0u;
            if (i < a.K) {
                const unsigned long long live = __ballot(c > i);
                if (!live) continue;
                unsigned before = 0;
                for (int w = 0; w < wave; ++w) before += wave_live[w][i];
                if (c > i && wanted) {
                    const unsigned long long pos = (unsigned long long)a.block_live[(block * 3 + ch) * a.K + i] + before +
                                                   (unsigned)__popcll(live & below);
                    const unsigned long long od = off[2 * (ch * a.K + i)], oc = off[2 * (ch * a.K + i) + 1];
                    rec[i] = (uint32_t)a.symbols[od + pos] | ((uint32_t)a.symbols[oc + pos] << 16);
                }
            }
        }
        if (wanted) {
            uint32_t* dst = choices + (t * 3 + ch) * a.K;
            if ((a.K & 3) == 0) {
#pragma unroll
                for (int v = 0; v < kMaxDeviceK / 4; ++v)
                    if (4 * v < a.K) reinterpret_cast<uint4*>(dst)[v] = make_uint4(rec[4 * v], rec[4 * v + 1], rec[4 * v + 2], rec[4 * v + 3]);
            } else {
#pragma unroll
                for (int i = 0; i < kMaxDeviceK; ++i)
                    if (i < a.K) dst[i] = rec[i];
            }
        }
    }
}

// The window of the tiles [t0, t1) in every stream, for a decode of a pixel rectangle (mpc_decode_regions_indexed).  Behind count
// and scan: block_live holds every 1024-tile block's offset in every stream pair, sizes the pairs' totals.  The rank of an edge t
// in pair (ch, i) = its block's offset + the tiles of that block in front of t with more than i atoms, by ballots as in the
// gather; an edge at the frame's end (t1 == tiles, which may lie behind the last block) has the pair's size.  One workgroup does
// both edges: a block-aligned t0 simply finds no tile in front of it.  Then a thread per stream writes (r0, r1) and the chunks
// that hold them -- or all chunks of a stream that cannot be cut.  Every value written is bounded here, by the host's n_chunks:
// the parse kernel trusts nothing else of it.
//
// kAux (index version 2): a stream with aux entries -- run-length packed, or a step-0 coefficient stream -- is cut as well, by its
// EXPANDED positions: c0 = the last checkpoint whose out[] is at or in front of r0, c1 = the first behind c0 whose out[] is at or
// behind r1, else n_chunks; nothing if r0 == r1.  Two binary searches over the stream's own n_chunks entries, which the host has
// checked (out[0] = 0, strictly increasing, <= expect); the entry and exit values go to the stream's WindowSpan, cut once more.
template <bool kAux>
__global__ __launch_bounds__(kBlockTiles) void mp_window_rank_kernel(const WindowArgs w)
{
    __shared__ unsigned rank[2][3 * kMaxDeviceK];
    const StreamArgs& a = w.sa;
    const int lane = threadIdx.x & 63, pairs = 3 * a.K;
    for (int e = 0; e < 2; ++e) {
        const long long edge = e ? w.t1 : w.t0;                   // 0 <= edge <= tiles (the host)
        const bool at_end = edge >= a.tiles;                      // uniform
        const long long b = at_end ? 0 : edge / kBlockTiles;      // < blocks
        if ((int)threadIdx.x < pairs) rank[e][threadIdx.x] = at_end ? a.sizes[threadIdx.x] : a.block_live[b * pairs + threadIdx.x];
        __syncthreads();
        if (at_end) continue;
        const long long t = b * kBlockTiles + threadIdx.x;
        const bool front = t < edge;                              // then t < tiles
        if (!__ballot(front)) continue;                           // a wave behind the edge adds nothing
        for (int ch = 0; ch < 3; ++ch) {
            const int c = front ? min((int)a.counts[t * 3 + ch], a.K) : 0;
#pragma unroll
            for (int i = 0; i < kMaxDeviceK; ++i)
                if (i < a.K) {
                    const unsigned long long live = __ballot(c > i);
                    if (lane == 0 && live) atomicAdd(&rank[e][ch * a.K + i], (unsigned)__popcll(live));
                }
        }
    }
    __syncthreads();
    const int s = threadIdx.x;                                    // stream 2 * pair + (0 deltaId | 1 intCoeff)
    if (s >= 2 * pairs) return;
    const unsigned long long r0 = rank[0][s >> 1], r1 = rank[1][s >> 1] > r0 ? rank[1][s >> 1] : r0;
    const unsigned n_chunks = w.parse[s + 1].n_chunks;
    const bool whole = w.parse_all || (w.unpack[s].flags & kUnpackPacked) != 0u || s % (2 * a.K) == 1;
    const unsigned long long first = r0 / w.interval, behind = (r1 + w.interval - 1) / w.interval;
    WindowStream out;
    out.r0 = r0;
    out.r1 = r1;
    out.c0 = whole ? 0u : (unsigned)(first < n_chunks ? first : n_chunks);
    out.c1 = whole ? n_chunks : (unsigned)(behind < n_chunks ? behind : n_chunks);
    if (kAux) {
        WindowSpan sp{};
        const unsigned long long off = w.aux_off[s];                // s < 6K
        if (!w.parse_all && off != ~0ull && n_chunks) {
            // entry j of the stream: aux[2 * (off + j)], [+ 1], j < n_chunks: the host laid n_chunks entries out for it
            const unsigned long long* e = w.aux + 2 * off;
            const unsigned long long n_coded = w.parse[s + 1].n_coded, expect = w.parse[s + 1].expect;
            unsigned c0 = 0, c1 = 0;
            if (r0 < r1) {
                unsigned lo = 0, hi = n_chunks;                     // out[lo] <= r0 (out[0] = 0), out[hi] > r0 or hi = n_chunks
                while (hi - lo > 1) {
                    const unsigned mid = lo + (hi - lo) / 2;        // 0 < mid < n_chunks
                    if (e[2 * (unsigned long long)mid] <= r0) lo = mid; else hi = mid;
                }
                c0 = lo;
                hi = n_chunks;                                      // out[lo] < r1 (out[c0] <= r0 < r1), out[hi] >= r1 or hi = n_chunks
                while (hi - lo > 1) {
                    const unsigned mid = lo + (hi - lo) / 2;
                    if (e[2 * (unsigned long long)mid] >= r1) hi = mid; else lo = mid;
                }
                c1 = hi;                                            // c0 < c1 <= n_chunks
            }
            out.c0 = c0;
            out.c1 = c1;
            const unsigned long long s1 = (unsigned long long)c1 * w.interval;
            sp.s0 = (unsigned long long)c0 * w.interval;           // <= n_coded: c0 < n_chunks
            sp.s1 = s1 < n_coded ? s1 : n_coded;
            const unsigned long long o0 = e[2 * (unsigned long long)c0], w0 = e[2 * (unsigned long long)c0 + 1];       // c0 < n_chunks
            sp.out0 = o0 < expect ? o0 : expect;
            sp.state0 = (unsigned)(w0 >> 32) < 2u ? (unsigned)(w0 >> 32) : 2u;
            sp.prev0 = (unsigned)(w0 & 0xFFFFu);
            sp.dc0 = (unsigned)((w0 >> 16) & 0xFFFFu);
            sp.out1 = expect;
            sp.flags = kSpanCut;
            if (c1 < n_chunks) {
                const unsigned long long o1 = e[2 * (unsigned long long)c1], w1 = e[2 * (unsigned long long)c1 + 1];
                sp.out1 = o1 < expect ? o1 : expect;
                sp.state1 = (unsigned)(w1 >> 32);
                sp.prev1 = (unsigned)(w1 & 0xFFFFu);
                sp.dc1 = (unsigned)((w1 >> 16) & 0xFFFFu);
                sp.flags |= kSpanCheck;
            }
            if (sp.out1 < sp.out0) sp.out1 = sp.out0;
        }
        w.span[s] = sp;
    }
    w.window[s] = out;
}

__global__ __launch_bounds__(256) void mp_stream_dc_kernel(const StreamArgs a)
{
    for (int ch = 0; ch < 3; ++ch) {
        const unsigned n = a.sizes[ch * a.K];
        const uint16_t* src = a.dc_tmp + (long long)ch * a.tiles;
        uint16_t* dst = a.symbols + a.stream_off[2 * (ch * a.K) + 1];
        for (unsigned long long j = (unsigned long long)blockIdx.x * 256 + threadIdx.x; j < n; j += (unsigned long long)gridDim.x * 256) {
            const int32_t v = src[j], prev = j ? (int32_t)src[j - 1] : 0;
            const int32_t d = v - prev;
            dst[j] = (uint16_t)(((uint32_t)d << 1) ^ (uint32_t)(d >> 31));     // zigzagEncode, BitBuffer.h:116
        }
    }
}

// A row stripe's records (tile t = tx * rows + ty_local, the order mpc_encode_tiles_device writes a stripe in) copied to their
// places in a whole frame's records (t = tx * tiles_y + row_begin + ty_local): the step between the stripe exchange of the
// multi-GPU path and the stream assembly, which reads whole frames in the reference's tile order (CompressedImage.cpp:535-537).
// Both sides are runs of rows * 3K words per tile column: coalesced reads and writes.
__global__ __launch_bounds__(256) void mp_interleave_stripe_kernel(const uint16_t* __restrict__ part_counts, const uint32_t* __restrict__ part_choices,
                                                                   int tiles_x, int tiles_y, int row_begin, int rows, int K,
                                                                   uint16_t* __restrict__ frame_counts, uint32_t* __restrict__ frame_choices)
{
    const long long words_per_col = (long long)rows * 3 * K, n_words = words_per_col * tiles_x;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (long long)gridDim.x * 256) {
        const long long tx = i / words_per_col, w = i - tx * words_per_col;
        frame_choices[(tx * tiles_y + row_begin) * 3 * K + w] = part_choices[i];
    }
    const long long halves_per_col = (long long)rows * 3, n_halves = halves_per_col * tiles_x;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_halves; i += (long long)gridDim.x * 256) {
        const long long tx = i / halves_per_col, w = i - tx * halves_per_col;
        frame_counts[(tx * tiles_y + row_begin) * 3 + w] = part_counts[i];
    }
}

// The records of the tile grid [tx0, tx1) x [ty0, ty1) of a frame as the frame of that grid alone (a transcode: the container of a
// rectangle from the source's records): tile (tx - tx0) * nty + (ty - ty0) takes the first min(count, steps) records of tile
// tx * tiles_y + ty, the steps behind them zero.  A tile column's rows are contiguous on both sides, as for the stripes above, so a
// thread per OUTPUT word reads and writes consecutive words across a wave whatever K is.  Every address comes from the grid: a
// count above K is clamped to K where it is used and sets *error, and the host refuses the frame.
__global__ __launch_bounds__(256) void mp_crop_records_kernel(const uint16_t* __restrict__ counts, const uint32_t* __restrict__ choices,
                                                              int tiles_y, int tx0, int ty0, int ncols, int nty, int K, int steps,
                                                              uint16_t* __restrict__ out_counts, uint32_t* __restrict__ out_choices,
                                                              int* __restrict__ error)
{
    const int halves_per_col = nty * 3, words_per_col = halves_per_col * K;      // < 2^31 (the launcher)
    const long long n_words = (long long)words_per_col * ncols, n_halves = (long long)halves_per_col * ncols;
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < n_words; o += (long long)gridDim.x * 256) {
        const int col = (int)(o / words_per_col), w = (int)(o - (long long)col * words_per_col);
        const int tc = w / K, i = w - tc * K;                             // tile-channel of the column's rows, step
        const long long first = ((long long)(tx0 + col) * tiles_y + ty0) * 3;    // the column's first tile-channel in the source
        int c = counts[first + tc];
        if (c > K) c = K;
        if (c > steps) c = steps;
        out_choices[o] = i < c ? choices[first * K + w] : 0u;
    }
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < n_halves; o += (long long)gridDim.x * 256) {
        const int col = (int)(o / halves_per_col), tc = (int)(o - (long long)col * halves_per_col);
        int c = counts[((long long)(tx0 + col) * tiles_y + ty0) * 3 + tc];
        if (c > K) {
            *error = 1;
            c = K;
        }
        out_counts[o] = (uint16_t)(c < steps ? c : steps);
    }
}

int launch_crop_records(const uint16_t* counts, const uint32_t* choices, int tiles_x, int tiles_y, int tx0, int ty0, int tx1, int ty1, int K,
                        int steps, uint16_t* out_counts, uint32_t* out_choices, int* error, void* stream_)
{
    if (tx0 < 0 || ty0 < 0 || tx0 >= tx1 || ty0 >= ty1 || tx1 > tiles_x || ty1 > tiles_y || K < 1 || K > kMaxDeviceK || steps < 1)
        return (int)hipErrorInvalidValue;
    const int ncols = tx1 - tx0, nty = ty1 - ty0;
    if ((long long)nty * 3 * K >= (1LL << 31)) return (int)hipErrorInvalidValue;
    const long long n_words = (long long)nty * 3 * K * ncols;
    const unsigned blocks = (unsigned)((n_words + 255) / 256 < 4096 ? (n_words + 255) / 256 : 4096);
    hipLaunchKernelGGL(mp_crop_records_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream_), counts, choices, tiles_y, tx0, ty0,
                       ncols, nty, K, steps < K ? steps : K, out_counts, out_choices, error);
    return (int)hipGetLastError();
}

// The inverse move (a compose: a container from rectangles of containers): the records of the grid of ncols x nty tiles at (stx0, sty0)
// of one frame into the grid of the same size at (dtx0, dty0) of another, both in whole-frame layout.  A tile column's rows are
// contiguous on both sides, so a thread per word of the grid reads and writes consecutive words across a wave whatever K is.  Records
// below the count are copied, the steps from the count to K are written as zero: garbage behind a source count is not carried over.
// owner: null, or one word per destination tile; a tile is then written only where owner[t] == part, so the pastes of one owner map
// write disjoint tiles.  Every address comes from the two grids: a count above K is clamped to K where it is used and sets *error.
__global__ __launch_bounds__(256) void mp_paste_records_kernel(const uint16_t* __restrict__ src_counts, const uint32_t* __restrict__ src_choices,
                                                               int src_tiles_y, int stx0, int sty0, int ncols, int nty, int K,
                                                               uint16_t* __restrict__ dst_counts, uint32_t* __restrict__ dst_choices,
                                                               int dst_tiles_y, int dtx0, int dty0, const int32_t* __restrict__ owner, int part,
                                                               int* __restrict__ error)
{
    const int halves_per_col = nty * 3, words_per_col = halves_per_col * K;      // < 2^31 (the launcher)
    const long long n_words = (long long)words_per_col * ncols, n_halves = (long long)halves_per_col * ncols;
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < n_words; o += (long long)gridDim.x * 256) {
        const int col = (int)(o / words_per_col), w = (int)(o - (long long)col * words_per_col);
        const int tc = w / K, i = w - tc * K;                             // tile-channel of the column's rows, step
        const long long to_tile = (long long)(dtx0 + col) * dst_tiles_y + dty0;  // the column's first tile on either side
        if (owner && owner[to_tile + tc / 3] != part) continue;
        const long long from = ((long long)(stx0 + col) * src_tiles_y + sty0) * 3;
        int c = src_counts[from + tc];
        if (c > K) c = K;
        dst_choices[to_tile * 3 * K + w] = i < c ? src_choices[from * K + w] : 0u;
    }
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < n_halves; o += (long long)gridDim.x * 256) {
        const int col = (int)(o / halves_per_col), tc = (int)(o - (long long)col * halves_per_col);
        const long long to_tile = (long long)(dtx0 + col) * dst_tiles_y + dty0;
        if (owner && owner[to_tile + tc / 3] != part) continue;
        int c = src_counts[((long long)(stx0 + col) * src_tiles_y + sty0) * 3 + tc];
        if (c > K) {
            *error = 1;
            c = K;
        }
        dst_counts[to_tile * 3 + tc] = (uint16_t)c;
    }
}

int launch_paste_records(const uint16_t* src_counts, const uint32_t* src_choices, int src_tiles_x, int src_tiles_y, int stx0, int sty0, int ncols,
                         int nty, int K, uint16_t* dst_counts, uint32_t* dst_choices, int dst_tiles_x, int dst_tiles_y, int dtx0, int dty0,
                         const int32_t* owner, int part, int* error, void* stream_)
{
    if (ncols < 1 || nty < 1 || K < 1 || K > kMaxDeviceK || stx0 < 0 || sty0 < 0 || dtx0 < 0 || dty0 < 0) return (int)hipErrorInvalidValue;
    if (ncols > src_tiles_x - stx0 || nty > src_tiles_y - sty0 || ncols > dst_tiles_x - dtx0 || nty > dst_tiles_y - dty0)
        return (int)hipErrorInvalidValue;
    if ((long long)nty * 3 * K >= (1LL << 31)) return (int)hipErrorInvalidValue;
    const long long n_words = (long long)nty * 3 * K * ncols;
    const unsigned blocks = (unsigned)((n_words + 255) / 256 < 4096 ? (n_words + 255) / 256 : 4096);
    hipLaunchKernelGGL(mp_paste_records_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream_), src_counts, src_choices, src_tiles_y,
                       stx0, sty0, ncols, nty, K, dst_counts, dst_choices, dst_tiles_y, dtx0, dty0, owner, part, error);
    return (int)hipGetLastError();
}

// A call's quantiser table to its device slot.  The table travels in the kernel's argument block, which the launch copies before it
// returns: the caller's memory may go away at once, and nothing waits for the stream as a copy from pageable memory does.
__global__ __launch_bounds__(64) void mp_quant_table_kernel(const QuantTable t, double* dst, int n)
{
    for (int i = threadIdx.x; i < n; i += 64) dst[i] = t.q[i];
}

int launch_quant_table(const double* quant, int K, double* dst, void* stream_)
{
    if (!quant || !dst || K < 1 || K > kMaxDeviceK) return (int)hipErrorInvalidValue;
    QuantTable t{};
    for (int i = 0; i < 3 * K; ++i) t.q[i] = quant[i];
    hipLaunchKernelGGL(mp_quant_table_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream_), t, dst, 3 * K);
    return (int)hipGetLastError();
}

int launch_interleave_stripe(const uint16_t* part_counts, const uint32_t* part_choices, int tiles_x, int tiles_y, int row_begin, int rows,
                             int K, uint16_t* frame_counts, uint32_t* frame_choices, void* stream_)
{
    if (tiles_x < 1 || rows < 1 || row_begin < 0 || row_begin + rows > tiles_y || K < 1 || K > kMaxDeviceK) return (int)hipErrorInvalidValue;
    const long long n_words = (long long)rows * 3 * K * tiles_x;
    const unsigned blocks = (unsigned)((n_words + 255) / 256 < 4096 ? (n_words + 255) / 256 : 4096);
    hipLaunchKernelGGL(mp_interleave_stripe_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream_), part_counts, part_choices,
                       tiles_x, tiles_y, row_begin, rows, K, frame_counts, frame_choices);
    return (int)hipGetLastError();
}

int launch_stream_gather(const StreamArgs& a, uint32_t* choices, void* stream_)
{
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const int blocks = (int)((a.tiles + kBlockTiles - 1) / kBlockTiles);
    if (blocks < 1 || a.K < 1 || a.K > kMaxDeviceK) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(mp_stream_count_kernel, dim3((unsigned)blocks), dim3(kBlockTiles), 0, s, a);
    hipLaunchKernelGGL(mp_stream_scan_kernel, dim3((unsigned)(3 * a.K)), dim3(64), 0, s, a, blocks);
    hipLaunchKernelGGL(mp_stream_gather_kernel<false>, dim3((unsigned)blocks), dim3(kBlockTiles), 0, s, a, choices, 0u, 0LL, 0LL);
    return (int)hipGetLastError();
}

int launch_window_rank(const WindowArgs& w, void* stream_)
{
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const StreamArgs& a = w.sa;
    const int blocks = (int)((a.tiles + kBlockTiles - 1) / kBlockTiles);
    if (blocks < 1 || a.K < 1 || a.K > kMaxDeviceK || w.interval < 1 || w.t0 < 0 || w.t0 >= w.t1 || w.t1 > a.tiles) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(mp_stream_count_kernel, dim3((unsigned)blocks), dim3(kBlockTiles), 0, s, a);
    hipLaunchKernelGGL(mp_stream_scan_kernel, dim3((unsigned)(3 * a.K)), dim3(64), 0, s, a, blocks);
    if (w.span) {
        if (!w.aux || !w.aux_off) return (int)hipErrorInvalidValue;
        hipLaunchKernelGGL(mp_window_rank_kernel<true>, dim3(1), dim3(kBlockTiles), 0, s, w);
    } else
        hipLaunchKernelGGL(mp_window_rank_kernel<false>, dim3(1), dim3(kBlockTiles), 0, s, w);
    return (int)hipGetLastError();
}

int launch_stream_gather_window(const StreamArgs& a, uint32_t* choices, long long t0, long long t1, void* stream_)
{
    hipStream_t s = static_cast<hipStream_t>(stream_);
    if (a.K < 1 || a.K > kMaxDeviceK || t0 < 0 || t0 >= t1 || t1 > a.tiles) return (int)hipErrorInvalidValue;
    const long long first = t0 / kBlockTiles, behind = (t1 + kBlockTiles - 1) / kBlockTiles;
    hipLaunchKernelGGL(mp_stream_gather_kernel<true>, dim3((unsigned)(behind - first)), dim3(kBlockTiles), 0, s, a, choices, (unsigned)first, t0, t1);
    return (int)hipGetLastError();
}

int launch_stream_scan(const StreamArgs& a, int pairs, int blocks, void* stream_)
{
    if (blocks < 1 || a.K < 1 || a.K > kMaxDeviceK || pairs < 1 || pairs > 3 * a.K) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(mp_stream_scan_kernel, dim3((unsigned)pairs), dim3(64), 0, static_cast<hipStream_t>(stream_), a, blocks);
    return (int)hipGetLastError();
}

size_t stream_workspace_words(long long tiles, int K)
{
    const long long blocks = (tiles + kBlockTiles - 1) / kBlockTiles;
    return (size_t)(blocks * 3 * K);
}

int launch_stream_assembly(const StreamArgs& a, void* stream_)
{
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const int blocks = (int)((a.tiles + kBlockTiles - 1) / kBlockTiles);
    if (blocks < 1 || a.K < 1 || a.K > kMaxDeviceK) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(mp_stream_count_kernel, dim3((unsigned)blocks), dim3(kBlockTiles), 0, s, a);
    hipLaunchKernelGGL(mp_stream_scan_kernel, dim3((unsigned)(3 * a.K)), dim3(64), 0, s, a, blocks);
    hipLaunchKernelGGL(mp_stream_scatter_kernel, dim3((unsigned)blocks), dim3(kBlockTiles), 0, s, a);
    hipLaunchKernelGGL(mp_stream_dc_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace mpc
