// mp_delta.hip -- product: the delta encoder's kernels (include/mpcodec.h, "delta"; DESIGN.md 4, "Encoder: changed tiles only").
//
// A tile's records depend on that tile's pixels alone, so a frame that differs from the last one in a few tiles needs the pursuit for
// those tiles only.  Three byte shufflers around the unchanged tile encoder:
//   diff     the new frame against the session's kept copy: a flag per tile, the kept copy brought up to date; then flags -> the
//            ascending list of changed tiles (count per 1024-tile block, mp_stream_scan_kernel over the blocks, rank by ballots)
//   pack     the listed tiles side by side in a small frame of whole tiles, which the tile encoder takes as an ordinary frame
//   scatter  that frame's records to the listed tiles' places in the whole frame's records
// and, for the receiver of a delta stream (include/mpcodec.h, "patch"), the pack's inverse:
//   unpack   a decoded packed frame's tiles to the listed tiles' places in the receiver's kept frame, cut to the image
// The diff is the hot one and purely bandwidth-bound: it reads both frames once.  A tile's pixel row is 24 bytes = three 8-byte chunks;
// a thread owns one chunk column of a strip of 64 horizontally adjacent tiles over the tile's 8 pixel rows, so a wave reads 512
// contiguous bytes of a pixel row per load, 8 independent loads per frame in flight, and a chunk is written back only where it differs.
// With a change tolerance ("Encoder: a change tolerance") mp_tile_diff_tol_kernel takes its place: the same strip, a
// tile's summed squared difference against the tolerance, and the kept copy written in changed tiles only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mp_device.h"

namespace mpc {

namespace {
constexpr int kDiffTiles = 64;                  // tiles of one tile row per workgroup
constexpr int kDiffThreads = 3 * kDiffTiles;    // a thread per 8-byte chunk of the strip's pixel rows
constexpr int kListBlock = 1024;                // tiles per workgroup of the flags -> list kernels (thread = tile)

__host__ __device__ inline long long list_blocks(long long tiles) { return (tiles + kListBlock - 1) / kListBlock; }
}  // namespace

// kWords: both frames' bases and strides are multiples of 8 and so is 3 * width: every chunk is whole and 8-byte aligned on both
// sides.  Else byte by byte, a chunk cut at the row's end: bytes behind 3 * width are never read.
template <bool kWords>
__global__ __launch_bounds__(kDiffThreads) void mp_tile_diff_kernel(uint8_t* __restrict__ kept, const uint8_t* __restrict__ rgb, int width,
                                                                    int height, long long row_stride, int tiles_x, int tiles_y, int strips,
                                                                    uint8_t* __restrict__ flags)
{
    __shared__ unsigned changed[kDiffTiles];
    const int ty = blockIdx.x / strips, tx0 = (blockIdx.x - ty * strips) * kDiffTiles;
    if (threadIdx.x < kDiffTiles) changed[threadIdx.x] = 0u;
    __syncthreads();
    const long long row_bytes = 3LL * width;
    const long long b0 = 24LL * tx0 + 8LL * threadIdx.x;             // the chunk's first byte in its pixel row
    const int y0 = ty * 8, rows = height - y0 < 8 ? height - y0 : 8;
    bool differs = false;
    if (b0 < row_bytes) {
        if (kWords) {
            uint2 fresh[8], old[8];
#pragma unroll
            for (int r = 0; r < 8; ++r)
                if (r < rows) {
                    fresh[r] = *reinterpret_cast<const uint2*>(rgb + (long long)(y0 + r) * row_stride + b0);
                    old[r] = *reinterpret_cast<const uint2*>(kept + (long long)(y0 + r) * row_bytes + b0);
                }
#pragma unroll
            for (int r = 0; r < 8; ++r)
                if (r < rows && (fresh[r].x != old[r].x || fresh[r].y != old[r].y)) {
                    differs = true;
                    *reinterpret_cast<uint2*>(kept + (long long)(y0 + r) * row_bytes + b0) = fresh[r];
                }
        } else {
            const int nb = row_bytes - b0 < 8 ? (int)(row_bytes - b0) : 8;
            for (int r = 0; r < rows; ++r) {
                const uint8_t* p = rgb + (long long)(y0 + r) * row_stride + b0;
                uint8_t* q = kept + (long long)(y0 + r) * row_bytes + b0;
                for (int j = 0; j < nb; ++j) {
                    const uint8_t v = p[j];
                    if (v != q[j]) {
                        differs = true;
                        q[j] = v;
                    }
                }
            }
        }
    }
    if (differs) changed[threadIdx.x / 3] = 1u;                      // every writer writes 1
    __syncthreads();
    if (threadIdx.x < kDiffTiles && tx0 + (int)threadIdx.x < tiles_x)
        flags[(long long)(tx0 + (int)threadIdx.x) * tiles_y + ty] = (uint8_t)changed[threadIdx.x];
}

// The diff with a tolerance (host_delta.h: changed_tiles_tolerance): the same strip, the same threads, the same 16 loads in flight,
// but a tile's verdict needs the whole tile, so nothing is written before it.  A thread sums the squared byte differences of its 8 x 8
// bytes -- per 32-bit word sum a^2 + sum b^2 - 2 sum ab, three v_dot4_u32_u8, at most 2 * 64 * 255^2 in the first accumulator -- and
// leaves the sum in LDS; a tile's three threads lie side by side but a tile can straddle two waves (64 is no multiple of 3), so they
// meet there and not in a cross-lane add.  Behind the barrier every thread adds its tile's three sums itself: one barrier, no atomic,
// no zeroing pass.  Only a changed tile's chunk columns are written, whole; a held or equal tile's kept pixels stay as they are.
// sse: NULL or one value per tile.  totals: NULL or {held tiles, the sum of their sse}, zeroed by the launch; a strip's 64 tiles are
// wave 0's lanes, which adds them up and sends one pair of atomics a workgroup that holds any.
__device__ inline void sq_diff_word(unsigned a, unsigned b, unsigned& squares, unsigned& cross)
{
    squares = __builtin_amdgcn_udot4(a, a, squares, false);
    squares = __builtin_amdgcn_udot4(b, b, squares, false);
    cross = __builtin_amdgcn_udot4(a, b, cross, false);
}

template <bool kWords>
__global__ __launch_bounds__(kDiffThreads) void mp_tile_diff_tol_kernel(uint8_t* __restrict__ kept, const uint8_t* __restrict__ rgb, int width,
                                                                        int height, long long row_stride, int tiles_x, int tiles_y, int strips,
                                                                        unsigned tolerance, uint8_t* __restrict__ flags,
                                                                        uint32_t* __restrict__ sse, unsigned long long* __restrict__ totals)
{
    __shared__ unsigned part[kDiffThreads];
    const int ty = blockIdx.x / strips, tx0 = (blockIdx.x - ty * strips) * kDiffTiles;
    const long long row_bytes = 3LL * width;
    const long long b0 = 24LL * tx0 + 8LL * threadIdx.x;             // the chunk's first byte in its pixel row
    const int y0 = ty * 8, rows = height - y0 < 8 ? height - y0 : 8;
    const bool inside = b0 < row_bytes;
    const int nb = !inside ? 0 : row_bytes - b0 < 8 ? (int)(row_bytes - b0) : 8;
    uint2 fresh[8];
    unsigned sum = 0u;
    if (inside) {
        if (kWords) {
            uint2 old[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                fresh[r] = old[r] = make_uint2(0u, 0u);
                if (r < rows) {
                    fresh[r] = *reinterpret_cast<const uint2*>(rgb + (long long)(y0 + r) * row_stride + b0);
                    old[r] = *reinterpret_cast<const uint2*>(kept + (long long)(y0 + r) * row_bytes + b0);
                }
            }
            unsigned squares = 0u, cross = 0u;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                sq_diff_word(fresh[r].x, old[r].x, squares, cross);
                sq_diff_word(fresh[r].y, old[r].y, squares, cross);
            }
            sum = squares - 2u * cross;
        } else {
            for (int r = 0; r < rows; ++r) {
                const uint8_t* p = rgb + (long long)(y0 + r) * row_stride + b0;
                const uint8_t* q = kept + (long long)(y0 + r) * row_bytes + b0;
                for (int j = 0; j < nb; ++j) {
                    const int diff = (int)p[j] - (int)q[j];
                    sum += (unsigned)(diff * diff);
                }
            }
        }
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    const int mine = 3 * (int)(threadIdx.x / 3);
    if (inside && part[mine] + part[mine + 1] + part[mine + 2] > tolerance) {
        if (kWords) {
#pragma unroll
            for (int r = 0; r < 8; ++r)
                if (r < rows) *reinterpret_cast<uint2*>(kept + (long long)(y0 + r) * row_bytes + b0) = fresh[r];
        } else {
            for (int r = 0; r < rows; ++r) {
                const uint8_t* p = rgb + (long long)(y0 + r) * row_stride + b0;
                uint8_t* q = kept + (long long)(y0 + r) * row_bytes + b0;
                for (int j = 0; j < nb; ++j) q[j] = p[j];
            }
        }
    }
    if (threadIdx.x < kDiffTiles) {                                  // wave 0, a lane per tile of the strip
        const unsigned tile_sse = part[3 * threadIdx.x] + part[3 * threadIdx.x + 1] + part[3 * threadIdx.x + 2];
        if (tx0 + (int)threadIdx.x < tiles_x) {
            const long long t = (long long)(tx0 + (int)threadIdx.x) * tiles_y + ty;
            flags[t] = tile_sse > tolerance ? 1 : 0;
            if (sse) sse[t] = tile_sse;
        }
        if (totals) {                                                // a tile behind tiles_x has no bytes: its sum is 0
            const bool held = tile_sse != 0u && tile_sse <= tolerance;
            const unsigned long long who = __ballot(held);
            unsigned held_sse = held ? tile_sse : 0u;                // 64 tiles: below 2^30
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) held_sse += __shfl_xor(held_sse, d);
            if (threadIdx.x == 0 && who) {
                atomicAdd(&totals[0], (unsigned long long)__popcll(who));
                atomicAdd(&totals[1], (unsigned long long)held_sse);
            }
        }
    }
}

// flags -> per block of 1024 tiles the number set, at block_live[3 * block]: column 0 of a StreamArgs table with K = 1, which
// mp_stream_scan_kernel turns into the blocks' offsets and the total
__global__ __launch_bounds__(kListBlock) void mp_tile_flag_count_kernel(const uint8_t* __restrict__ flags, long long tiles,
                                                                        unsigned* __restrict__ block_live)
{
    __shared__ unsigned total;
    if (threadIdx.x == 0) total = 0u;
    __syncthreads();
    const long long t = (long long)blockIdx.x * kListBlock + threadIdx.x;
    const unsigned long long live = __ballot(t < tiles && flags[t < tiles ? t : 0] != 0);
    if ((threadIdx.x & 63) == 0 && live) atomicAdd(&total, (unsigned)__popcll(live));
    __syncthreads();
    if (threadIdx.x == 0) block_live[3LL * blockIdx.x] = total;
}

// the list: a set tile's place is its block's offset + the set tiles of the waves in front + its rank in its wave -- ascending in t
__global__ __launch_bounds__(kListBlock) void mp_tile_list_kernel(const uint8_t* __restrict__ flags, long long tiles,
                                                                  const unsigned* __restrict__ block_live, int32_t* __restrict__ list)
{
    __shared__ unsigned wave_live[kListBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long t = (long long)blockIdx.x * kListBlock + threadIdx.x;
    const bool set = t < tiles && flags[t < tiles ? t : 0] != 0;
    const unsigned long long live = __ballot(set);
    if (lane == 0) wave_live[wave] = (unsigned)__popcll(live);
    __syncthreads();
    if (!set) return;
    unsigned at = block_live[3LL * blockIdx.x];
    for (int w = 0; w < wave; ++w) at += wave_live[w];
    list[at + (unsigned)__popcll(live & ((1ULL << lane) - 1ULL))] = (int32_t)t;
}

// A thread per 8-byte chunk of the packed frame.  kWords: the source's base and stride are multiples of 8; a chunk that lies whole
// inside its pixel row is then one 8-byte load, and every other chunk (and every chunk without kWords) is gathered byte by byte
template <bool kWords>
__global__ __launch_bounds__(256) void mp_tile_pack_kernel(const uint8_t* __restrict__ rgb, int width, int height, long long row_stride,
                                                           int tiles_y, long long tiles, const int32_t* __restrict__ list, long long n, int rows,
                                                           int cols, uint8_t* __restrict__ packed, long long packed_stride)
{
    const long long chunks_per_row = 3LL * cols, total = chunks_per_row * 8 * rows, row_bytes = 3LL * width;
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < total; o += (long long)gridDim.x * 256) {
        const long long py = o / chunks_per_row;
        const int k = (int)(o - py * chunks_per_row), txp = k / 3, part = k - 3 * txp;
        const long long j = (long long)txp * rows + (py >> 3);
        uint2 v = make_uint2(0u, 0u);                                // black: outside the image, a padding tile
        const long long t = j < n ? (long long)list[j] : -1;
        if (t >= 0 && t < tiles) {
            const long long tx = t / tiles_y, y = (t - tx * tiles_y) * 8 + (py & 7), b0 = 24 * tx + 8 * part;
            if (y < height && b0 < row_bytes) {
                const uint8_t* p = rgb + y * row_stride + b0;
                if (kWords && b0 + 8 <= row_bytes) {
                    v = *reinterpret_cast<const uint2*>(p);
                } else {
                    const int nb = row_bytes - b0 < 8 ? (int)(row_bytes - b0) : 8;
                    unsigned long long bits = 0;
                    for (int b = 0; b < nb; ++b) bits |= (unsigned long long)p[b] << (8 * b);
                    v = make_uint2((unsigned)bits, (unsigned)(bits >> 32));
                }
            }
        }
        *reinterpret_cast<uint2*>(packed + py * packed_stride + 8LL * k) = v;
    }
}

// The pack kernel's inverse, for the receiver of a delta stream (mpcodec_patch.cpp): a thread per 8-byte chunk of the packed frame.
// The chunk of listed tile j at packed tile (j / rows, j % rows) goes to tile list[j] of the frame, cut to the image: nothing at or
// behind 3 * width of a row, no row at or below height, nothing for a padding tile (j >= n).  kWords: the frame's base and stride are
// multiples of 8; a chunk that lies whole inside its pixel row is then one 8-byte store, and every other chunk (and every chunk
// without kWords) is written byte by byte.  An entry outside [0, tiles) writes nothing and sets *error: every address comes from
// list[j] after its check against `tiles`
template <bool kWords>
__global__ __launch_bounds__(256) void mp_tile_unpack_kernel(const uint8_t* __restrict__ packed, long long packed_stride,
                                                             const int32_t* __restrict__ list, long long n, int rows, int cols,
                                                             uint8_t* __restrict__ rgb, int width, int height, long long row_stride,
                                                             int tiles_y, long long tiles, int* __restrict__ error)
{
    const long long chunks_per_row = 3LL * cols, total = chunks_per_row * 8 * rows, row_bytes = 3LL * width;
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < total; o += (long long)gridDim.x * 256) {
        const long long py = o / chunks_per_row;
        const int k = (int)(o - py * chunks_per_row), txp = k / 3, part = k - 3 * txp;
        const long long j = (long long)txp * rows + (py >> 3);
        if (j >= n) continue;                                        // a padding tile
        const long long t = list[j];
        if (t < 0 || t >= tiles) {
            *error = 1;
            continue;
        }
        const long long tx = t / tiles_y, y = (t - tx * tiles_y) * 8 + (py & 7), b0 = 24 * tx + 8 * part;
        if (y >= height || b0 >= row_bytes) continue;                // the black fill of a ragged tile
        const uint2 v = *reinterpret_cast<const uint2*>(packed + py * packed_stride + 8LL * k);
        uint8_t* p = rgb + y * row_stride + b0;
        if (kWords && b0 + 8 <= row_bytes) {
            *reinterpret_cast<uint2*>(p) = v;
        } else {
            const int nb = row_bytes - b0 < 8 ? (int)(row_bytes - b0) : 8;
            const unsigned long long bits = (unsigned long long)v.x | (unsigned long long)v.y << 32;
            for (int b = 0; b < nb; ++b) p[b] = (uint8_t)(bits >> (8 * b));
        }
    }
}

// A thread per record word, then per count.  The encoder zeroes the entries beyond a count, so a plain copy carries no garbage.
// Every address comes from list[j] after its check against `tiles`
__global__ __launch_bounds__(256) void mp_tile_scatter_records_kernel(const uint16_t* __restrict__ packed_counts,
                                                                      const uint32_t* __restrict__ packed_choices,
                                                                      const int32_t* __restrict__ list, long long n, int K,
                                                                      uint16_t* __restrict__ counts, uint32_t* __restrict__ choices,
                                                                      long long tiles, int* __restrict__ error)
{
    const int words = 3 * K;
    const long long n_words = n * words, n_halves = n * 3;
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < n_words; o += (long long)gridDim.x * 256) {
        const long long j = o / words, t = list[j];
        if (t < 0 || t >= tiles) continue;
        choices[t * words + (o - j * words)] = packed_choices[o];
    }
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < n_halves; o += (long long)gridDim.x * 256) {
        const long long j = o / 3, t = list[j];
        if (t < 0 || t >= tiles) {
            *error = 1;
            continue;
        }
        counts[t * 3 + (o - j * 3)] = packed_counts[o];
    }
}

size_t tile_diff_scratch_bytes(long long tiles)
{
    return (size_t)((tiles + 255) & ~255LL) + sizeof(unsigned) * 3 * (size_t)list_blocks(tiles);
}

int launch_tile_diff(uint8_t* kept, const uint8_t* rgb, int width, int height, size_t row_stride, int32_t* list, int32_t* count, void* scratch,
                     void* stream_)
{
    hipStream_t s = static_cast<hipStream_t>(stream_);
    if (!kept || !rgb || !list || !count || !scratch || width < 1 || height < 1 || row_stride < 3 * (size_t)width) return (int)hipErrorInvalidValue;
    const long long tiles_x = ((long long)width + 7) / 8, tiles_y = ((long long)height + 7) / 8, tiles = tiles_x * tiles_y;
    const long long strips = (tiles_x + kDiffTiles - 1) / kDiffTiles;
    if (tiles >= (1LL << 31) || strips * tiles_y >= (1LL << 31)) return (int)hipErrorInvalidValue;
    uint8_t* flags = static_cast<uint8_t*>(scratch);
    unsigned* block_live = tile_diff_block_live(scratch, tiles);
    const size_t row_bytes = 3 * (size_t)width;
    const bool words = ((reinterpret_cast<uintptr_t>(kept) | reinterpret_cast<uintptr_t>(rgb) | row_stride | row_bytes) & 7) == 0;
    const dim3 grid((unsigned)(strips * tiles_y));
    if (words)
        hipLaunchKernelGGL(mp_tile_diff_kernel<true>, grid, dim3(kDiffThreads), 0, s, kept, rgb, width, height, (long long)row_stride, (int)tiles_x,
                           (int)tiles_y, (int)strips, flags);
    else
        hipLaunchKernelGGL(mp_tile_diff_kernel<false>, grid, dim3(kDiffThreads), 0, s, kept, rgb, width, height, (long long)row_stride, (int)tiles_x,
                           (int)tiles_y, (int)strips, flags);
    return launch_tile_flags_list(flags, tiles, block_live, list, count, s);
}

int launch_tile_diff_tolerance(uint8_t* kept, const uint8_t* rgb, int width, int height, size_t row_stride, uint32_t tolerance, int32_t* list,
                               int32_t* count, uint32_t* sse, unsigned long long* totals, void* scratch, void* stream_)
{
    hipStream_t s = static_cast<hipStream_t>(stream_);
    if (!kept || !rgb || !list || !count || !scratch || width < 1 || height < 1 || row_stride < 3 * (size_t)width) return (int)hipErrorInvalidValue;
    const long long tiles_x = ((long long)width + 7) / 8, tiles_y = ((long long)height + 7) / 8, tiles = tiles_x * tiles_y;
    const long long strips = (tiles_x + kDiffTiles - 1) / kDiffTiles;
    if (tiles >= (1LL << 31) || strips * tiles_y >= (1LL << 31)) return (int)hipErrorInvalidValue;
    uint8_t* flags = static_cast<uint8_t*>(scratch);
    unsigned* block_live = tile_diff_block_live(scratch, tiles);
    const size_t row_bytes = 3 * (size_t)width;
    const bool words = ((reinterpret_cast<uintptr_t>(kept) | reinterpret_cast<uintptr_t>(rgb) | row_stride | row_bytes) & 7) == 0;
    const dim3 grid((unsigned)(strips * tiles_y));
    if (totals)
        if (const hipError_t e = hipMemsetAsync(totals, 0, 2 * sizeof(unsigned long long), s); e != hipSuccess) return (int)e;
    if (words)
        hipLaunchKernelGGL(mp_tile_diff_tol_kernel<true>, grid, dim3(kDiffThreads), 0, s, kept, rgb, width, height, (long long)row_stride,
                           (int)tiles_x, (int)tiles_y, (int)strips, tolerance, flags, sse, totals);
    else
        hipLaunchKernelGGL(mp_tile_diff_tol_kernel<false>, grid, dim3(kDiffThreads), 0, s, kept, rgb, width, height, (long long)row_stride,
                           (int)tiles_x, (int)tiles_y, (int)strips, tolerance, flags, sse, totals);
    return launch_tile_flags_list(flags, tiles, block_live, list, count, s);
}

unsigned* tile_diff_block_live(void* scratch, long long tiles)
{
    return reinterpret_cast<unsigned*>(static_cast<uint8_t*>(scratch) + ((tiles + 255) & ~255LL));
}

int launch_tile_flags_list(const uint8_t* flags, long long tiles, unsigned* block_live, int32_t* list, int32_t* count, void* stream_)
{
    hipStream_t s = static_cast<hipStream_t>(stream_);
    if (!flags || !block_live || !list || !count || tiles < 1 || tiles >= (1LL << 31)) return (int)hipErrorInvalidValue;
    const int blocks = (int)list_blocks(tiles);
    hipLaunchKernelGGL(mp_tile_flag_count_kernel, dim3((unsigned)blocks), dim3(kListBlock), 0, s, flags, tiles, block_live);
    StreamArgs a{};
    a.K = 1;
    a.block_live = block_live;
    a.sizes = reinterpret_cast<unsigned*>(count);
    if (const int e = launch_stream_scan(a, 1, blocks, s); e != 0) return e;
    hipLaunchKernelGGL(mp_tile_list_kernel, dim3((unsigned)blocks), dim3(kListBlock), 0, s, flags, tiles, block_live, list);
    return (int)hipGetLastError();
}

int launch_tile_pack(const uint8_t* rgb, int width, int height, size_t row_stride, const int32_t* list, long long n, int rows, int cols,
                     uint8_t* packed, size_t packed_stride, void* stream_)
{
    if (!rgb || !list || !packed || width < 1 || height < 1 || row_stride < 3 * (size_t)width || n < 1 || rows < 1 || cols < 1) return (int)hipErrorInvalidValue;
    if (n > (long long)rows * cols || packed_stride < 24 * (size_t)cols || ((reinterpret_cast<uintptr_t>(packed) | packed_stride) & 7) != 0)
        return (int)hipErrorInvalidValue;
    const long long tiles_y = ((long long)height + 7) / 8, tiles = (((long long)width + 7) / 8) * tiles_y;
    if (tiles >= (1LL << 31)) return (int)hipErrorInvalidValue;
    const long long total = 3LL * cols * 8 * rows;
    const unsigned blocks = (unsigned)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    const bool words = ((reinterpret_cast<uintptr_t>(rgb) | row_stride) & 7) == 0;
    hipStream_t s = static_cast<hipStream_t>(stream_);
    if (words)
        hipLaunchKernelGGL(mp_tile_pack_kernel<true>, dim3(blocks), dim3(256), 0, s, rgb, width, height, (long long)row_stride, (int)tiles_y, tiles, list,
                           n, rows, cols, packed, (long long)packed_stride);
    else
        hipLaunchKernelGGL(mp_tile_pack_kernel<false>, dim3(blocks), dim3(256), 0, s, rgb, width, height, (long long)row_stride, (int)tiles_y, tiles, list,
                           n, rows, cols, packed, (long long)packed_stride);
    return (int)hipGetLastError();
}

int launch_tile_unpack(const uint8_t* packed, size_t packed_stride, const int32_t* list, long long n, int rows, int cols, uint8_t* rgb, int width,
                       int height, size_t row_stride, int* error, void* stream_)
{
    if (!packed || !list || !rgb || !error || width < 1 || height < 1 || row_stride < 3 * (size_t)width || n < 1 || rows < 1 || cols < 1)
        return (int)hipErrorInvalidValue;
    if (n > (long long)rows * cols || packed_stride < 24 * (size_t)cols || ((reinterpret_cast<uintptr_t>(packed) | packed_stride) & 7) != 0)
        return (int)hipErrorInvalidValue;
    const long long tiles_y = ((long long)height + 7) / 8, tiles = (((long long)width + 7) / 8) * tiles_y;
    if (tiles >= (1LL << 31)) return (int)hipErrorInvalidValue;
    const long long total = 3LL * cols * 8 * rows;
    const unsigned blocks = (unsigned)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    const bool words = ((reinterpret_cast<uintptr_t>(rgb) | row_stride) & 7) == 0;
    hipStream_t s = static_cast<hipStream_t>(stream_);
    if (words)
        hipLaunchKernelGGL(mp_tile_unpack_kernel<true>, dim3(blocks), dim3(256), 0, s, packed, (long long)packed_stride, list, n, rows, cols, rgb, width,
                           height, (long long)row_stride, (int)tiles_y, tiles, error);
    else
        hipLaunchKernelGGL(mp_tile_unpack_kernel<false>, dim3(blocks), dim3(256), 0, s, packed, (long long)packed_stride, list, n, rows, cols, rgb, width,
                           height, (long long)row_stride, (int)tiles_y, tiles, error);
    return (int)hipGetLastError();
}

int launch_tile_scatter_records(const uint16_t* packed_counts, const uint32_t* packed_choices, const int32_t* list, long long n, int K,
                                uint16_t* counts, uint32_t* choices, long long tiles, int* error, void* stream_)
{
    if (!packed_counts || !packed_choices || !list || !counts || !choices || !error || n < 1 || tiles < 1 || tiles >= (1LL << 31) || K < 1 ||
        K > kMaxDeviceK)
        return (int)hipErrorInvalidValue;
    const long long n_words = n * 3 * K;
    const unsigned blocks = (unsigned)((n_words + 255) / 256 < 4096 ? (n_words + 255) / 256 : 4096);
    hipLaunchKernelGGL(mp_tile_scatter_records_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream_), packed_counts, packed_choices,
                       list, n, K, counts, choices, tiles, error);
    return (int)hipGetLastError();
}

}  // namespace mpc
