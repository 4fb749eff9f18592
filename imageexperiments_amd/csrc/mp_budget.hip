// mp_budget.hip -- product: the rate control's kernels (include/mpcodec.h, "budget"; DESIGN.md 4, "Encoder: a byte budget").
//
// The container is layered by pursuit step and nothing reads a record beyond its count, so cutting a tile to its first n steps is a
// change of three counts.  Two kernels tell the search of mpc_encode_image_budget where to cut:
//   profile   per tile the decoder's squared error at every depth n = 0 ... K, from one replay of the records
//   allocate  per tile the depth that minimises distortion + multiplier * rate, the cut counts and the frame's totals
// Both are one wave per tile and bandwidth-light: the profile reads 3K record words, at most 3K dictionary rows of 64 values and
// 192 pixel bytes per tile, the allocation K + 1 words.  A third serves mpc_encode_image_quality ("quality"):
//   sweep     the allocation's totals at all 256 multipliers in one launch, thread = multiplier
// and two for a group of frames to one budget or one quality ("group"): the allocation and the sweep over up to eight frames a launch,
// the frame as blockIdx.y, every frame with its own weights.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "host_budget.h"
#include "mp_device.h"

namespace mpc {

namespace {
constexpr int kPixels = 64;             // an 8 x 8 tile: a row of the dictionary
constexpr int kProfileWaves = 4;        // tiles a workgroup works on at a time
constexpr int kAllocateWaves = 4;
}  // namespace

// --------------------------------------------------------------------------------------------------
// depth profile: one wave per tile, LANE = PIXEL, as in mp_decode_kernel.  The rows of all three channels' records are resolved
// once, the way reconstruct_tile_pixel (mp_kernels.hip) resolves them -- lane i takes record i, its choice by a wave scan over the
// zig-zag deltas, its row by the walk over the channel's base choices -- with one more condition: the base choice that unlocks a
// detail row must lie at a step below the record's own.  Then the row of record i is the same whatever depth >= i + 1 the tile is
// cut to, and the accumulation of depth n is a prefix of that of depth n + 1: the walk n = 1 ... K adds step n - 1 of every channel
// that has it (one rounding for the product, one for the sum, no FMA: reconstruct_tile_pixel's arithmetic in its order), and after
// each n RGBFromYUV's rounding and clamp, the integer dr^2 + dg^2 + db^2 of the pixels inside the frame and a wave sum give what
// mp_distortion_kernel gives for the counts cut to n.  Lane n keeps P[n]; depths above the tile's largest count repeat the last
// value; the tile's K + 1 words leave in one contiguous store.  A record whose row is not in the dictionary of its earlier steps
// (a forward reference, a choice outside the dictionary, a negative one) adds nothing and sets *error, and so does a count above
// K, which is used as K: every address comes from the tile grid and from rows checked against the block table.
// --------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(64 * kProfileWaves) void mp_depth_profile_kernel(const DictDevice dict, const ProfileParams p)
{
    constexpr bool kFast = std::is_same<T, float>::value;
    const T* const base_rows = reinterpret_cast<const T*>(kFast ? static_cast<const void*>(dict.base32) : static_cast<const void*>(dict.base));
    const T* const detail_rows = reinterpret_cast<const T*>(kFast ? static_cast<const void*>(dict.detail32) : static_cast<const void*>(dict.detail));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = p.K;
    const long long tiles = (long long)p.tiles_x * p.tiles_y;
    for (long long t = (long long)blockIdx.x * kProfileWaves + wave; t < tiles; t += (long long)gridDim.x * kProfileWaves) {
        uint32_t rec[3];
        long long row_at[3];            // element offset of this lane's record's row; -1: none
        int in_base[3], cnt[3];
        int deepest = 0;
        bool bad = false;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            int count = p.counts[t * 3 + ch];
            if (count > K) {
                count = K;
                bad = true;
            }
            cnt[ch] = count;
            deepest = count > deepest ? count : deepest;
            const uint32_t* recs = p.choices + (t * 3 + ch) * K;
            const uint32_t r = lane < count ? recs[lane] : 0u;
            const unsigned delta = r & 0xFFFFu;
            int choice = lane == 0 ? (int)delta : (int)((delta >> 1) ^ (0u - (delta & 1u)));
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(choice, o);
                if (lane >= o) choice += up;
            }
            long long at = -1;
            int base = 0;
            if (choice >= 0 && choice < dict.num_base) {
                at = (long long)choice * kPixels;
                base = 1;
            }
            int off = dict.num_base;
            bool open = lane < count && choice >= dict.num_base;
            for (int k = 0; k < count; ++k) {
                const int walk = __shfl(choice, k);
                if (walk >= 0 && walk < dict.num_base) {
                    const int rows = dict.block_rows[walk];
                    if (open && choice < off + rows) {
                        if (k < lane) at = ((long long)ch * dict.detail_rows + dict.block_row_off[walk] + (choice - off)) * kPixels;
                        open = false;
                    }
                    off += rows;
                }
            }
            if (lane < count && at < 0) bad = true;
            rec[ch] = r;
            row_at[ch] = at;
            in_base[ch] = base;
        }
        if (__any(bad ? 1 : 0) && lane == 0) *p.error = 1;
        const int tx = (int)(t / p.tiles_y), ty = (int)(t - (long long)tx * p.tiles_y);
        const int u = tx * 8 + (lane & 7), v = ty * 8 + (lane >> 3);
        const bool inside = u < p.width && v < p.height;
        int r0 = 0, g0 = 0, b0 = 0;
        if (inside) {
            const uint8_t* px = p.original + 3 * ((long long)v * p.width + u);
            r0 = px[0];
            g0 = px[1];
            b0 = px[2];
        }
        T acc[3] = {0, 0, 0};
        uint32_t mine = 0;
        int e = 0;
        for (int n = 0; n <= K; ++n) {
            if (n <= deepest) {                                     // uniform: every lane takes part in every exchange
                if (n >= 1) {
                    const int i = n - 1;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        if (i < cnt[ch]) {
                            const uint32_t ri = (uint32_t)__shfl((int)rec[ch], i);
                            const unsigned zz = ri >> 16;
                            const int q = (int)((zz >> 1) ^ (0u - (zz & 1u)));
                            const T coeff = (T)p.quant[ch * K + i] * (T)q;
                            const long long at = __shfl(row_at[ch], i);
                            const int from_base = __shfl(in_base[ch], i);
                            if (at >= 0) {
                                const T* row = (from_base ? base_rows : detail_rows) + at;
                                const T term = row[lane] * coeff;
                                acc[ch] = acc[ch] + term;
                            }
                        }
                    }
                }
                const double Y = (double)acc[0], U = (double)acc[1], V = (double)acc[2];
                double rr = __builtin_round(Y + 1.13983 * V);
                double gg = __builtin_round(Y - 0.39466 * U - 0.58060 * V);
                double bb = __builtin_round(Y + 2.03211 * U);
                rr = rr < 0.0 ? 0.0 : (rr > 255.0 ? 255.0 : rr);
                gg = gg < 0.0 ? 0.0 : (gg > 255.0 ? 255.0 : gg);
                bb = bb < 0.0 ? 0.0 : (bb > 255.0 ? 255.0 : bb);
                e = 0;
                if (inside) {
                    const int dr = (int)rr - r0, dg = (int)gg - g0, db = (int)bb - b0;
                    e = dr * dr + dg * dg + db * db;
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
            }
            if (lane == n) mine = (uint32_t)e;
        }
        if (lane <= K) p.profile[t * (K + 1) + lane] = mine;
    }
}

// --------------------------------------------------------------------------------------------------
// allocation: one wave per tile, lane n = depth n.  The K + 1 profile words of a tile are one coalesced load; the rate of a depth
// comes from the per-channel prefix sums of the weights, which the workgroup builds once in LDS from the weights in its arguments;
// J = P * 65536 + lambda * R (u64: P < 2^24, lambda < 2^35, R < 2^27).  The minimum is taken over the pair (J, n) in that order by a
// butterfly, so equal J leave the smallest n -- J has no six spare bits to pack n into.  Lanes above K hold J = 2^64 - 1, which no
// depth reaches.  Lanes 0 ... 2 store the cut counts, lane 0 the depth; a wave adds up its tiles' distortion, rate and records
// kept, the waves' sums meet in LDS, and threads 0 ... 2 add one total each to the frame's: one 64-bit integer atomic per total
// and workgroup, as in mp_distortion_kernel, so the totals do not depend on the schedule.  Every address comes from the tile grid;
// a count above K is used as K.
// kEmphasis (host_budget.h, "emphasis"): J = P * e[t] * 4096 + lambda * R, e[t] one byte per tile through emphasis_used, so no address
// comes from it; the totals keep the unweighted P.  P * 64 * 4096 < 2^42, so J stays below 2^63.  The plain kernel is the
// instantiation without it and reads no emphasis pointer: its code is what it was.
// --------------------------------------------------------------------------------------------------
template <bool kEmphasis>
__global__ __launch_bounds__(64 * kAllocateWaves) void mp_budget_allocate_kernel(const AllocateParams p)
{
    __shared__ uint32_t below[3][kMaxDeviceK + 1];                  // below[ch][m] = W[ch][0] + ... + W[ch][m - 1]
    __shared__ unsigned long long wave_sum[kAllocateWaves][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = p.K;
    if (threadIdx.x < 3) {
        uint32_t sum = 0;
        below[threadIdx.x][0] = 0;
        for (int i = 0; i < K; ++i) {
            sum += p.weights[threadIdx.x * K + i];
            below[threadIdx.x][i + 1] = sum;
        }
    }
    __syncthreads();
    unsigned long long distortion = 0, rate = 0, records = 0;
    for (long long t = (long long)blockIdx.x * kAllocateWaves + wave; t < p.tiles; t += (long long)gridDim.x * kAllocateWaves) {
        int cnt[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int count = p.counts[t * 3 + ch];
            cnt[ch] = count > K ? K : count;
        }
        unsigned long long factor = 0;
        if (kEmphasis) factor = (unsigned long long)emphasis_used(p.emphasis[t]) << kEmphasisShift;
        uint32_t P = 0, R = 0;
        unsigned long long J = ~0ull;
        if (lane <= K) {
            P = p.profile[t * (K + 1) + lane];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) R += below[ch][lane < cnt[ch] ? lane : cnt[ch]];
            J = (kEmphasis ? P * factor : (unsigned long long)P << 16) + p.lambda * R;
        }
        int depth = lane;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(J, o);
            const int other_depth = __shfl_xor(depth, o);
            if (other < J || (other == J && other_depth < depth)) {
                J = other;
                depth = other_depth;
            }
        }
        // every lane holds the winner; depth <= K because lane 0's J is below 2^63
        const uint32_t kept_P = (uint32_t)__shfl((int)P, depth), kept_R = (uint32_t)__shfl((int)R, depth);
        if (lane == 0) p.depth[t] = (uint8_t)depth;
        if (lane < 3) {
            const int mine = lane == 0 ? cnt[0] : lane == 1 ? cnt[1] : cnt[2];
            p.out_counts[t * 3 + lane] = (uint16_t)(mine < depth ? mine : depth);
        }
        distortion += kept_P;
        rate += kept_R;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) records += (unsigned)(cnt[ch] < depth ? cnt[ch] : depth);
    }
    if (lane == 0) {
        wave_sum[wave][0] = distortion;
        wave_sum[wave][1] = rate;
        wave_sum[wave][2] = records;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long total = 0;
        for (int w = 0; w < kAllocateWaves; ++w) total += wave_sum[w][threadIdx.x];
        if (total) atomicAdd(p.totals + threadIdx.x, total);
    }
}

// --------------------------------------------------------------------------------------------------
// sweep: the allocation's three totals at all 256 multipliers in one launch (host_budget.h: budget_sweep), the allocation kernel turned
// round: THREAD m = MULTIPLIER m, a workgroup of 256 threads holds the whole ladder.  L[m] = mant << shift with mant <= 15, and
// L * R = (mant * R) << shift in u64, exactly (R < 2^27).  A workgroup takes kSweepTiles consecutive tiles at a time -- their profile
// words are one contiguous run, loaded coalesced -- and stages per tile and depth n what does not depend on the multiplier: P * 65536,
// R[n] from the prefix sums in LDS, and the records kept, 16 bytes an entry.  Behind the barrier every thread walks the staged tiles
// serially, n = 0 ... K: every lane reads the same entry (an LDS broadcast), J = P * 65536 + L * R, and keeps the first strict
// minimum -- no butterfly, and the smallest n wins ties by construction.  It adds the winner's P, R and records to three u64
// accumulators that live in registers for the whole grid-stride loop.  At the end the 768 sums pass through LDS, so that a wave adds
// 64 consecutive words (512 contiguous bytes) per 64-bit integer atomic: 768 atomics a workgroup, at most kSweepGridCap workgroups
// whatever the frame.  The totals are integers and do not depend on the schedule.  Every address comes from the tile grid; a count
// above K is used as K.
// kEmphasis: the staged entry carries P * e[t] * 4096 and, since that no longer gives P back by a shift, the true P beside the records
// kept in one word -- P < 2^24, at most 3 * 32 = 96 records -- so an entry stays 16 bytes and the LDS budget is unchanged.  The walk is
// the same; the winner's true P is what the distortion total adds.  The plain kernel is the instantiation without it.
// --------------------------------------------------------------------------------------------------
namespace {
struct alignas(16) SweepEntry {
    unsigned long long scaled;          // P * 65536; with emphasis P * e * 4096
    uint32_t rate, kept;                // with emphasis: kept = records kept | P << 8
};
}  // namespace

template <bool kEmphasis>
__global__ __launch_bounds__(256) void mp_budget_sweep_kernel(const SweepParams p)
{
    __shared__ uint32_t below[3][kMaxDeviceK + 1];                  // below[ch][m] = W[ch][0] + ... + W[ch][m - 1]
    __shared__ SweepEntry staged[kSweepTiles * (kMaxDeviceK + 1)];
    __shared__ unsigned long long sums[3 * 256];
    const int m = threadIdx.x;
    const int K = p.K, depths = K + 1;
    if (m < 3) {
        uint32_t sum = 0;
        below[m][0] = 0;
        for (int i = 0; i < K; ++i) {
            sum += p.weights[m * K + i];
            below[m][i + 1] = sum;
        }
    }
    const unsigned mant = m == 0 ? 0u : 8u + (unsigned)(m - 1) % 8u;   // L[m] = mant << shift (host_budget.h: budget_lambda)
    const unsigned shift = m == 0 ? 0u : (unsigned)(m - 1) / 8u;
    unsigned long long distortion = 0, rate = 0, records = 0;
    const long long chunks = (p.tiles + kSweepTiles - 1) / kSweepTiles;
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const long long first = c * kSweepTiles;
        const int here = (int)(p.tiles - first < kSweepTiles ? p.tiles - first : kSweepTiles);
        __syncthreads();                                            // the walk before has read `staged`; the first time: `below` is built
        for (int e = m; e < here * depths; e += 256) {
            const int s = e / depths, n = e - s * depths;
            const long long t = first + s;
            uint32_t R = 0, kept = 0;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int count = p.counts[t * 3 + ch];
                const int cnt = count > K ? K : count;
                const int upto = n < cnt ? n : cnt;
                R += below[ch][upto];
                kept += (uint32_t)upto;
            }
            SweepEntry entry;
            const uint32_t P = p.profile[first * depths + e];
            if (kEmphasis) {
                entry.scaled = P * ((unsigned long long)emphasis_used(p.emphasis[t]) << kEmphasisShift);
                entry.kept = kept | P << 8;
            } else {
                entry.scaled = (unsigned long long)P << 16;
                entry.kept = kept;
            }
            entry.rate = R;
            staged[e] = entry;
        }
        __syncthreads();
        for (int s = 0; s < here; ++s) {
            const SweepEntry* tile = staged + s * depths;
            unsigned long long best = tile[0].scaled + (((unsigned long long)mant * tile[0].rate) << shift);
            int at = 0;
#pragma unroll 4
            for (int n = 1; n <= K; ++n) {
                const SweepEntry e = tile[n];
                const unsigned long long J = e.scaled + (((unsigned long long)mant * e.rate) << shift);
                if (J < best) {
                    best = J;
                    at = n;
                }
            }
            const SweepEntry won = tile[at];
            distortion += kEmphasis ? (unsigned long long)(won.kept >> 8) : won.scaled >> 16;
            rate += won.rate;
            records += kEmphasis ? won.kept & 0xFFu : won.kept;
        }
    }
    sums[3 * m] = distortion;
    sums[3 * m + 1] = rate;
    sums[3 * m + 2] = records;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const unsigned long long total = sums[k * 256 + m];
        if (total) atomicAdd(p.totals + k * 256 + m, total);
    }
}

// --------------------------------------------------------------------------------------------------
// mask to emphasis (host_budget.h: emphasis_from_mask): one pass over a u8 mask at pixel resolution.  A workgroup of 256 threads takes a
// block of 32 * kPix x kMaskTilesY tiles: thread x reads kPix neighbouring pixels of every pixel row of the block, so a wave's load is
// 64 * kPix consecutive bytes of one row.  kPix = 4 where the mask's base and stride are multiples of 4: one 32-bit load, taken only
// where all four pixels lie inside the frame -- the last pixels of a row whose width is no multiple of 4 come byte by byte, so the bytes
// between rows are never addressed; kPix = 1 for any other alignment.  A thread keeps the maximum of each tile row's eight pixel rows
// in a register, the 8 / kPix neighbouring lanes of one tile's columns (a tile never straddles a wave) meet in shuffles, and the maxima
// land in LDS so that the store runs along ty, the inner index of t = tx * tiles_y + ty.  Pixels right of the frame and below it count
// as 0, the identity of the maximum over u8; every address comes from the geometry.
// --------------------------------------------------------------------------------------------------
namespace {
constexpr int kMaskTilesY = 4;
}  // namespace

template <int kPix>
__global__ __launch_bounds__(256) void mp_emphasis_mask_kernel(const uint8_t* __restrict__ mask, int width, int height, size_t row_stride, int lo,
                                                               int hi, int tiles_x, int tiles_y, int across, uint8_t* __restrict__ emphasis)
{
    constexpr int kTilesX = 32 * kPix, kLanes = 8 / kPix;             // tile columns a workgroup takes; lanes that share a tile
    __shared__ uint8_t top[kTilesX][kMaskTilesY];
    const int bx = (int)(blockIdx.x % (unsigned)across), by = (int)(blockIdx.x / (unsigned)across);
    const int x = (bx * 256 + (int)threadIdx.x) * kPix;
    const int ty0 = by * kMaskTilesY;
#pragma unroll
    for (int r = 0; r < kMaskTilesY; ++r) {
        const int y0 = (ty0 + r) * 8;
        unsigned m = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int y = y0 + k;
            if (y < height) {
                const uint8_t* row = mask + (size_t)y * row_stride;
                if (kPix == 4 && x + 4 <= width) {
                    const unsigned v = *reinterpret_cast<const unsigned*>(row + x);
                    const unsigned a = v & 0xFFu, b = (v >> 8) & 0xFFu, c = (v >> 16) & 0xFFu, d = v >> 24;
                    const unsigned ab = a > b ? a : b, cd = c > d ? c : d, abcd = ab > cd ? ab : cd;
                    m = abcd > m ? abcd : m;
                } else {
#pragma unroll
                    for (int i = 0; i < kPix; ++i)
                        if (x + i < width) {
                            const unsigned v = row[x + i];
                            m = v > m ? v : m;
                        }
                }
            }
        }
#pragma unroll
        for (int o = 1; o < kLanes; o <<= 1) {
            const unsigned other = (unsigned)__shfl_xor((int)m, o);
            m = other > m ? other : m;
        }
        if (threadIdx.x % kLanes == 0) top[threadIdx.x / kLanes][r] = (uint8_t)m;
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < kTilesX * kMaskTilesY; i += 256) {
        const int cx = i / kMaskTilesY, cy = i % kMaskTilesY;
        const int tx = bx * kTilesX + cx, ty = ty0 + cy;
        if (tx < tiles_x && ty < tiles_y) emphasis[(size_t)tx * tiles_y + ty] = (uint8_t)(lo + ((hi - lo) * (int)top[cx][cy] + 127) / 255);
    }
}

// --------------------------------------------------------------------------------------------------
// a group of frames (host_budget.h: budget_allocate_group, budget_sweep_group; include/mpcodec.h, "group"): the allocation and the sweep
// over up to kGroupChunk frames of one geometry in one launch, siblings of the two kernels above, which stay the code they are.
// blockIdx.y = the frame, so a workgroup is FRAME-PURE: all its tiles are frame f's, its prefix sums in LDS come from frame f's weights
// (the chunk's weights travel in the arguments, kGroupChunk * 384 bytes), and its grid-stride loop runs over blockIdx.x inside that
// frame alone -- the sweep's staging run of kSweepTiles tiles is cut at the frame's last tile like the single frame's, never carried into
// the next frame.  Tile t of frame f is tile f * tiles + t of every array.  The allocation adds its three totals to totals[f][0 .. 2], the
// sweep its 768 to the one ladder all frames share: 64-bit integer atomics, so neither depends on the schedule.  Every address comes
// from the tile grid and the frame index; a count above K is used as K; an emphasis byte passes through emphasis_used.
// --------------------------------------------------------------------------------------------------
template <bool kEmphasis>
__global__ __launch_bounds__(64 * kAllocateWaves) void mp_budget_allocate_group_kernel(const AllocateGroupParams p)
{
    __shared__ uint32_t below[3][kMaxDeviceK + 1];                  // frame f's: below[ch][m] = W[f][ch][0] + ... + W[f][ch][m - 1]
    __shared__ unsigned long long wave_sum[kAllocateWaves][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = p.K;
    const int f = (int)blockIdx.y;                                  // < p.frames <= kGroupChunk: the launcher's grid
    const long long first = (long long)f * p.tiles;                 // the frame's first tile in every array
    if (threadIdx.x < 3) {
        const uint32_t* W = p.weights + f * 3 * kMaxDeviceK + threadIdx.x * K;
        uint32_t sum = 0;
        below[threadIdx.x][0] = 0;
        for (int i = 0; i < K; ++i) {
            sum += W[i];
            below[threadIdx.x][i + 1] = sum;
        }
    }
    __syncthreads();
    unsigned long long distortion = 0, rate = 0, records = 0;
    for (long long t = (long long)blockIdx.x * kAllocateWaves + wave; t < p.tiles; t += (long long)gridDim.x * kAllocateWaves) {
        const long long g = first + t;
        int cnt[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int count = p.counts[g * 3 + ch];
            cnt[ch] = count > K ? K : count;
        }
        unsigned long long factor = 0;
        if (kEmphasis) factor = (unsigned long long)emphasis_used(p.emphasis[g]) << kEmphasisShift;
        uint32_t P = 0, R = 0;
        unsigned long long J = ~0ull;
        if (lane <= K) {
            P = p.profile[g * (K + 1) + lane];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) R += below[ch][lane < cnt[ch] ? lane : cnt[ch]];
            J = (kEmphasis ? P * factor : (unsigned long long)P << 16) + p.lambda * R;
        }
        int depth = lane;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(J, o);
            const int other_depth = __shfl_xor(depth, o);
            if (other < J || (other == J && other_depth < depth)) {
                J = other;
                depth = other_depth;
            }
        }
        // every lane holds the winner; depth <= K because lane 0's J is below 2^63
        const uint32_t kept_P = (uint32_t)__shfl((int)P, depth), kept_R = (uint32_t)__shfl((int)R, depth);
        if (lane == 0) p.depth[g] = (uint8_t)depth;
        if (lane < 3) {
            const int mine = lane == 0 ? cnt[0] : lane == 1 ? cnt[1] : cnt[2];
            p.out_counts[g * 3 + lane] = (uint16_t)(mine < depth ? mine : depth);
        }
        distortion += kept_P;
        rate += kept_R;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) records += (unsigned)(cnt[ch] < depth ? cnt[ch] : depth);
    }
    if (lane == 0) {
        wave_sum[wave][0] = distortion;
        wave_sum[wave][1] = rate;
        wave_sum[wave][2] = records;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long total = 0;
        for (int w = 0; w < kAllocateWaves; ++w) total += wave_sum[w][threadIdx.x];
        if (total) atomicAdd(p.totals + 3 * f + threadIdx.x, total);
    }
}

template <bool kEmphasis>
__global__ __launch_bounds__(256) void mp_budget_sweep_group_kernel(const SweepGroupParams p)
{
    __shared__ uint32_t below[3][kMaxDeviceK + 1];                  // frame f's
    __shared__ SweepEntry staged[kSweepTiles * (kMaxDeviceK + 1)];
    __shared__ unsigned long long sums[3 * 256];
    const int m = threadIdx.x;
    const int K = p.K, depths = K + 1;
    const int f = (int)blockIdx.y;                                  // < p.frames <= kGroupChunk: the launcher's grid
    const long long frame_first = (long long)f * p.tiles;
    if (m < 3) {
        const uint32_t* W = p.weights + f * 3 * kMaxDeviceK + m * K;
        uint32_t sum = 0;
        below[m][0] = 0;
        for (int i = 0; i < K; ++i) {
            sum += W[i];
            below[m][i + 1] = sum;
        }
    }
    const unsigned mant = m == 0 ? 0u : 8u + (unsigned)(m - 1) % 8u;   // L[m] = mant << shift (host_budget.h: budget_lambda)
    const unsigned shift = m == 0 ? 0u : (unsigned)(m - 1) / 8u;
    unsigned long long distortion = 0, rate = 0, records = 0;
    const long long chunks = (p.tiles + kSweepTiles - 1) / kSweepTiles;   // of this frame: the last run ends at the frame's last tile
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const long long in_frame = c * kSweepTiles;
        const int here = (int)(p.tiles - in_frame < kSweepTiles ? p.tiles - in_frame : kSweepTiles);
        const long long first = frame_first + in_frame;
        __syncthreads();                                            // the walk before has read `staged`; the first time: `below` is built
        for (int e = m; e < here * depths; e += 256) {
            const int s = e / depths, n = e - s * depths;
            const long long g = first + s;
            uint32_t R = 0, kept = 0;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int count = p.counts[g * 3 + ch];
                const int cnt = count > K ? K : count;
                const int upto = n < cnt ? n : cnt;
                R += below[ch][upto];
                kept += (uint32_t)upto;
            }
            SweepEntry entry;
            const uint32_t P = p.profile[first * depths + e];
            if (kEmphasis) {
                entry.scaled = P * ((unsigned long long)emphasis_used(p.emphasis[g]) << kEmphasisShift);
                entry.kept = kept | P << 8;
            } else {
                entry.scaled = (unsigned long long)P << 16;
                entry.kept = kept;
            }
            entry.rate = R;
            staged[e] = entry;
        }
        __syncthreads();
        for (int s = 0; s < here; ++s) {
            const SweepEntry* tile = staged + s * depths;
            unsigned long long best = tile[0].scaled + (((unsigned long long)mant * tile[0].rate) << shift);
            int at = 0;
#pragma unroll 4
            for (int n = 1; n <= K; ++n) {
                const SweepEntry e = tile[n];
                const unsigned long long J = e.scaled + (((unsigned long long)mant * e.rate) << shift);
                if (J < best) {
                    best = J;
                    at = n;
                }
            }
            const SweepEntry won = tile[at];
            distortion += kEmphasis ? (unsigned long long)(won.kept >> 8) : won.scaled >> 16;
            rate += won.rate;
            records += kEmphasis ? won.kept & 0xFFu : won.kept;
        }
    }
    sums[3 * m] = distortion;
    sums[3 * m + 1] = rate;
    sums[3 * m + 2] = records;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const unsigned long long total = sums[k * 256 + m];
        if (total) atomicAdd(p.totals + k * 256 + m, total);
    }
}

int launch_depth_profile(const DictDevice& dict, const ProfileParams& p, void* stream)
{
    if (p.K < 1 || p.K > kMaxDeviceK || p.width < 1 || p.height < 1 || p.tiles_x != (p.width + 7) / 8 || p.tiles_y != (p.height + 7) / 8)
        return (int)hipErrorInvalidValue;
    const long long tiles = (long long)p.tiles_x * p.tiles_y;
    const long long groups = (tiles + kProfileWaves - 1) / kProfileWaves;
    const unsigned blocks = (unsigned)(groups < 4096 ? groups : 4096);
    if (p.fast) hipLaunchKernelGGL(mp_depth_profile_kernel<float>, dim3(blocks), dim3(64 * kProfileWaves), 0, (hipStream_t)stream, dict, p);
    else hipLaunchKernelGGL(mp_depth_profile_kernel<double>, dim3(blocks), dim3(64 * kProfileWaves), 0, (hipStream_t)stream, dict, p);
    return (int)hipGetLastError();
}

int launch_budget_allocate(const AllocateParams& p, void* stream)
{
    if (p.K < 1 || p.K > kMaxDeviceK || p.tiles < 1) return (int)hipErrorInvalidValue;
    const long long groups = (p.tiles + kAllocateWaves - 1) / kAllocateWaves;
    const unsigned blocks = (unsigned)(groups < 4096 ? groups : 4096);
    if (p.emphasis) hipLaunchKernelGGL(mp_budget_allocate_kernel<true>, dim3(blocks), dim3(64 * kAllocateWaves), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(mp_budget_allocate_kernel<false>, dim3(blocks), dim3(64 * kAllocateWaves), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

int launch_budget_sweep(const SweepParams& p, void* stream)
{
    if (p.K < 1 || p.K > kMaxDeviceK || p.tiles < 1) return (int)hipErrorInvalidValue;
    const long long chunks = (p.tiles + kSweepTiles - 1) / kSweepTiles;
    const unsigned blocks = (unsigned)(chunks < kSweepGridCap ? chunks : kSweepGridCap);
    if (p.emphasis) hipLaunchKernelGGL(mp_budget_sweep_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(mp_budget_sweep_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

namespace {
// frames [begin, begin + n) of a group's weights [frames][3][K] to a launch's arguments
void chunk_weights(const uint32_t* weights, int begin, int n, int K, uint32_t* out)
{
    for (int f = 0; f < n; ++f)
        for (int i = 0; i < 3 * K; ++i) out[f * 3 * kMaxDeviceK + i] = weights[((size_t)(begin + f) * 3) * K + i];
}
bool group_fits(int frames, long long tiles, int K)
{
    return K >= 1 && K <= kMaxDeviceK && frames >= 1 && tiles >= 1 && tiles * 3 * frames < (1LL << 31);
}
}  // namespace

int launch_budget_allocate_group(const uint32_t* profile, const uint16_t* counts, const uint8_t* emphasis, int frames, long long tiles, int K,
                                 const uint32_t* weights, unsigned long long lambda, uint8_t* depth, uint16_t* out_counts,
                                 unsigned long long* totals, void* stream)
{
    if (!group_fits(frames, tiles, K) || !profile || !counts || !weights || !depth || !out_counts || !totals) return (int)hipErrorInvalidValue;
    const long long groups = (tiles + kAllocateWaves - 1) / kAllocateWaves;
    const unsigned blocks = (unsigned)(groups < 4096 ? groups : 4096);
    for (int begin = 0; begin < frames; begin += kGroupChunk) {
        const long long first = (long long)begin * tiles;
        AllocateGroupParams p{};
        p.profile = profile + first * (K + 1);
        p.counts = counts + first * 3;
        p.tiles = tiles;
        p.K = K;
        p.frames = frames - begin < kGroupChunk ? frames - begin : kGroupChunk;
        p.lambda = lambda;
        p.depth = depth + first;
        p.out_counts = out_counts + first * 3;
        p.totals = totals + 3 * begin;
        p.emphasis = emphasis ? emphasis + first : nullptr;
        chunk_weights(weights, begin, p.frames, K, p.weights);
        const dim3 grid(blocks, (unsigned)p.frames);
        if (emphasis) hipLaunchKernelGGL(mp_budget_allocate_group_kernel<true>, grid, dim3(64 * kAllocateWaves), 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL(mp_budget_allocate_group_kernel<false>, grid, dim3(64 * kAllocateWaves), 0, (hipStream_t)stream, p);
        const int err = (int)hipGetLastError();
        if (err != 0) return err;
    }
    return 0;
}

int launch_budget_sweep_group(const uint32_t* profile, const uint16_t* counts, const uint8_t* emphasis, int frames, long long tiles, int K,
                              const uint32_t* weights, unsigned long long* totals, void* stream)
{
    if (!group_fits(frames, tiles, K) || !profile || !counts || !weights || !totals) return (int)hipErrorInvalidValue;
    const long long chunks = (tiles + kSweepTiles - 1) / kSweepTiles;
    for (int begin = 0; begin < frames; begin += kGroupChunk) {
        const long long first = (long long)begin * tiles;
        SweepGroupParams p{};
        p.profile = profile + first * (K + 1);
        p.counts = counts + first * 3;
        p.tiles = tiles;
        p.K = K;
        p.frames = frames - begin < kGroupChunk ? frames - begin : kGroupChunk;
        p.totals = totals;
        p.emphasis = emphasis ? emphasis + first : nullptr;
        chunk_weights(weights, begin, p.frames, K, p.weights);
        // at most kSweepGridCap workgroups a launch, as for one frame: each adds 768 totals once
        const long long cap = kSweepGridCap / p.frames;
        const dim3 grid((unsigned)(chunks < cap ? chunks : cap), (unsigned)p.frames);
        if (emphasis) hipLaunchKernelGGL(mp_budget_sweep_group_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL(mp_budget_sweep_group_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, p);
        const int err = (int)hipGetLastError();
        if (err != 0) return err;
    }
    return 0;
}

int launch_emphasis_mask(const uint8_t* mask, int width, int height, size_t row_stride, int lo, int hi, uint8_t* emphasis, void* stream)
{
    if (!mask || !emphasis || width < 1 || height < 1 || row_stride < (size_t)width || lo < 1 || hi < lo || hi > kEmphasisMax)
        return (int)hipErrorInvalidValue;
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    const bool words = ((reinterpret_cast<uintptr_t>(mask) | row_stride) & 3) == 0;
    const int per_group = 32 * (words ? 4 : 1);
    const int across = (tiles_x + per_group - 1) / per_group, down = (tiles_y + kMaskTilesY - 1) / kMaskTilesY;
    const long long groups = (long long)across * down;
    if (groups >= (1LL << 31)) return (int)hipErrorInvalidValue;
    if (words)
        hipLaunchKernelGGL(mp_emphasis_mask_kernel<4>, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, mask, width, height, row_stride, lo, hi,
                           tiles_x, tiles_y, across, emphasis);
    else
        hipLaunchKernelGGL(mp_emphasis_mask_kernel<1>, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, mask, width, height, row_stride, lo, hi,
                           tiles_x, tiles_y, across, emphasis);
    return (int)hipGetLastError();
}

}  // namespace mpc
