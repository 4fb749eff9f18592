// mp_rate.hip -- product: the kernels of a delta stream to a byte budget (include/mpcodec.h, "rate"; DESIGN.md 4, "Delta stream to
// a byte budget").
//
// A sender that cuts its patches to a byte budget has to know what the receiver holds of each tile: the map sent[t], a depth per
// tile.  Four kernels work on that state, all byte shufflers or one coalesced load per tile:
//   owed flags  a tile whose sent depth is below its records' is owed; the flag joins the diff's per-tile flags, so the existing
//               flags -> list kernels (mp_delta.hip) make the ascending candidate list; per tile the floor and must bytes beside it
//   gather      the scatter turned round, with a cut: the listed tiles' records out of the whole frame's, cut to a depth per tile, as
//               the records of the packed frame of those tiles; everything above a cut and every padding tile is zero
//   allocate    mp_budget_allocate_kernel (mp_budget.hip) with a floor: a tile that need not be sent may only gain depth, and
//               staying where it is costs no rate
//   commit      sent[t] = the depth tile t was sent at, for the tiles of the patch the search returns
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_budget.h"
#include "mp_device.h"

namespace mpc {

namespace {
constexpr int kAllocateWaves = 4;
}  // namespace

// A thread per tile.  Every address comes from the tile grid; a count above K is used as K
__global__ __launch_bounds__(256) void mp_owed_flags_kernel(const uint8_t* __restrict__ sent, const uint16_t* __restrict__ counts, long long tiles,
                                                            int K, uint8_t* __restrict__ flags, uint8_t* __restrict__ floor,
                                                            uint8_t* __restrict__ must)
{
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < tiles; t += (long long)gridDim.x * 256) {
        int full = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int count = counts[t * 3 + ch];
            const int used = count > K ? K : count;
            full = used > full ? used : full;
        }
        const int have = sent[t];
        const bool changed = flags[t] != 0;
        must[t] = changed ? 1 : 0;
        floor[t] = changed ? 0 : (uint8_t)have;
        flags[t] = (uint8_t)((changed ? 1 : 0) | (have < full ? 2 : 0));
    }
}

namespace {
// packed tile j -> its candidate c and tile t; false: a padding tile, or an entry outside its range (then *bad)
__device__ inline bool gather_source(const GatherParams& p, long long j, long long* c_out, long long* t_out, bool* bad)
{
    if (j >= p.n) return false;
    const long long c = p.idx ? (long long)p.idx[j] : j;
    if (c < 0 || c >= p.m) {
        *bad = true;
        return false;
    }
    const long long t = p.list[c];
    if (t < 0 || t >= p.tiles) {
        *bad = true;
        return false;
    }
    *c_out = c;
    *t_out = t;
    return true;
}

// the count packed tile-channel (j, ch) receives
__device__ inline int gather_count(const GatherParams& p, long long c, long long t, int ch)
{
    const int count = p.counts[t * 3 + ch];
    const int cut = p.depth ? (int)p.depth[c] : p.K;
    const int used = count > p.K ? p.K : count;
    return used < cut ? used : cut;
}
}  // namespace

// A thread per 16-byte piece (four record words) of the packed records, then per count.  kVec: K is a multiple of 4 and both record
// bases are 16-byte aligned, so a piece lies in one tile-channel and is one 16-byte load and one 16-byte store; else word by word,
// the last piece cut at the end.  Every address comes from idx[j] and list[c] after their checks
template <bool kVec>
__global__ __launch_bounds__(256) void mp_gather_records_kernel(const GatherParams p)
{
    const int K = p.K;
    const long long n_words = p.padded * 3 * K, n_pieces = (n_words + 3) >> 2, n_halves = p.padded * 3;
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < n_pieces; o += (long long)gridDim.x * 256) {
        const long long w0 = o << 2;
        bool bad = false;
        if (kVec) {
            const long long jc = w0 / K, j = jc / 3;
            const int i0 = (int)(w0 - jc * K), ch = (int)(jc - j * 3);
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            long long c = 0, t = 0;
            if (gather_source(p, j, &c, &t, &bad)) {
                const int keep = gather_count(p, c, t, ch);
                if (i0 < keep) {
                    v = *reinterpret_cast<const uint4*>(p.choices + (t * 3 + ch) * K + i0);
                    if (i0 + 1 >= keep) v.y = 0u;
                    if (i0 + 2 >= keep) v.z = 0u;
                    if (i0 + 3 >= keep) v.w = 0u;
                }
            }
            *reinterpret_cast<uint4*>(p.out_choices + w0) = v;
        } else {
            long long at = -1, c = 0, t = 0;                         // the packed tile the source was last resolved for
            bool have = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long w = w0 + k;
                if (w >= n_words) break;
                const long long jc = w / K, j = jc / 3;
                const int i = (int)(w - jc * K), ch = (int)(jc - j * 3);
                if (j != at) {
                    have = gather_source(p, j, &c, &t, &bad);
                    at = j;
                }
                uint32_t v = 0u;
                if (have && i < gather_count(p, c, t, ch)) v = p.choices[(t * 3 + ch) * K + i];
                p.out_choices[w] = v;
            }
        }
    }
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < n_halves; o += (long long)gridDim.x * 256) {
        const long long j = o / 3;
        const int ch = (int)(o - j * 3);
        bool bad = false;
        long long c = 0, t = 0;
        int keep = 0;
        const bool have = gather_source(p, j, &c, &t, &bad);
        if (have) keep = gather_count(p, c, t, ch);
        if (bad) *p.error = 1;
        p.out_counts[o] = (uint16_t)keep;
        if (ch < 2 && p.tile_bytes[ch]) p.out_bytes[ch][j] = have ? p.tile_bytes[ch][t] : (uint8_t)0;
    }
}

// --------------------------------------------------------------------------------------------------
// allocation with a floor: mp_budget_allocate_kernel's shape -- one wave per candidate, lane n = depth n, the weights' prefix sums built
// once per workgroup in LDS, J = P * 65536 + lambda * R' in u64, a butterfly over the pair (J, n) so equal J leave the smallest n.
// A candidate that need not be sent (must == 0) may only take its floor or a depth above it, and its floor costs no rate: the
// receiver holds that much already.  A depth that is not allowed, and every lane above K, holds J = 2^64 - 1, which no allowed depth
// reaches (P < 2^24, lambda < 2^35, R < 2^27); the floor, used as K when above it, is always allowed, so the winner is an allowed
// depth.  Lanes 0 ... 2 store the cut counts, lane 0 the depth and the send byte; the four totals (distortion, rate, the records of the
// candidates sent, the candidates sent) meet in LDS and leave in one 64-bit integer atomic each per workgroup.
// kEmphasis (host_rate.h: budget_allocate_floor_emphasis): J = P * e * 4096 + lambda * R', e the byte of the candidate's tile --
// list[i], or i without a list -- through emphasis_used, the neutral value where that tile is outside [0, tiles): the list entry is
// checked before it becomes an address.  The totals keep the unweighted P.  The plain kernel is the instantiation without it.
// --------------------------------------------------------------------------------------------------
template <bool kEmphasis>
__global__ __launch_bounds__(64 * kAllocateWaves) void mp_budget_allocate_floor_kernel(const AllocateFloorParams p)
{
    __shared__ uint32_t below[3][kMaxDeviceK + 1];                  // below[ch][m] = W[ch][0] + ... + W[ch][m - 1]
    __shared__ unsigned long long wave_sum[kAllocateWaves][4];
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
    unsigned long long distortion = 0, rate = 0, records = 0, sent = 0;
    for (long long t = (long long)blockIdx.x * kAllocateWaves + wave; t < p.n; t += (long long)gridDim.x * kAllocateWaves) {
        int cnt[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int count = p.counts[t * 3 + ch];
            cnt[ch] = count > K ? K : count;
        }
        const bool must = p.must ? p.must[t] != 0 : true;
        int low = p.floor ? (int)p.floor[t] : 0;
        low = low > K ? K : low;
        unsigned long long factor = 0;
        if (kEmphasis) {
            const long long tile = p.list ? (long long)p.list[t] : t;
            factor = (unsigned long long)(tile >= 0 && tile < p.tiles ? emphasis_used(p.emphasis[tile]) : (uint32_t)kEmphasisNeutral) << kEmphasisShift;
        }
        uint32_t P = 0, R = 0;
        unsigned long long J = ~0ull;
        if (lane <= K && (must || lane >= low)) {
            P = p.profile[t * (K + 1) + lane];
            if (must || lane != low) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) R += below[ch][lane < cnt[ch] ? lane : cnt[ch]];
            }
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
        // every lane holds the winner, an allowed depth: lane `low`'s J is below 2^63
        const uint32_t kept_P = (uint32_t)__shfl((int)P, depth), kept_R = (uint32_t)__shfl((int)R, depth);
        const bool sends = must || depth > low;
        if (lane == 0) {
            p.depth[t] = (uint8_t)depth;
            p.send[t] = sends ? 1 : 0;
        }
        if (lane < 3) {
            const int mine = lane == 0 ? cnt[0] : lane == 1 ? cnt[1] : cnt[2];
            p.out_counts[t * 3 + lane] = (uint16_t)(mine < depth ? mine : depth);
        }
        distortion += kept_P;
        rate += kept_R;
        if (sends) {
            sent += 1;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) records += (unsigned)(cnt[ch] < depth ? cnt[ch] : depth);
        }
    }
    if (lane == 0) {
        wave_sum[wave][0] = distortion;
        wave_sum[wave][1] = rate;
        wave_sum[wave][2] = records;
        wave_sum[wave][3] = sent;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long total = 0;
        for (int w = 0; w < kAllocateWaves; ++w) total += wave_sum[w][threadIdx.x];
        if (total) atomicAdd(p.totals + threadIdx.x, total);
    }
}

// sent[list[c]] = depth ? depth[c] : K for the candidates c = idx ? idx[j] : j, j < n, that were sent.  The entries were the gather's:
// one outside its range is skipped
__global__ __launch_bounds__(256) void mp_sent_commit_kernel(const int32_t* __restrict__ list, long long m, const int32_t* __restrict__ idx,
                                                             const uint8_t* __restrict__ depth, long long n, int K, uint8_t* __restrict__ sent,
                                                             long long tiles)
{
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long long)gridDim.x * 256) {
        const long long c = idx ? (long long)idx[j] : j;
        if (c < 0 || c >= m) continue;
        const long long t = list[c];
        if (t < 0 || t >= tiles) continue;
        sent[t] = depth ? depth[c] : (uint8_t)K;
    }
}

int launch_sent_commit(const int32_t* list, long long m, const int32_t* idx, const uint8_t* depth, long long n, int K, uint8_t* sent,
                       long long tiles, void* stream)
{
    if (!list || !sent || m < 1 || n < 1 || (!idx && n > m) || tiles < 1 || K < 1 || K > kMaxDeviceK) return (int)hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(mp_sent_commit_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, list, m, idx, depth, n, K, sent, tiles);
    return (int)hipGetLastError();
}

int launch_owed_flags(const uint8_t* sent, const uint16_t* counts, long long tiles, int K, uint8_t* flags, uint8_t* floor, uint8_t* must,
                      void* stream)
{
    if (!sent || !counts || !flags || !floor || !must || tiles < 1 || tiles >= (1LL << 31) || K < 1 || K > kMaxDeviceK) return (int)hipErrorInvalidValue;
    const long long groups = (tiles + 255) / 256;
    const unsigned blocks = (unsigned)(groups < 4096 ? groups : 4096);
    hipLaunchKernelGGL(mp_owed_flags_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, sent, counts, tiles, K, flags, floor, must);
    return (int)hipGetLastError();
}

int launch_gather_records(const GatherParams& p, void* stream)
{
    if (!p.counts || !p.choices || !p.list || !p.out_counts || !p.out_choices || !p.error || p.K < 1 || p.K > kMaxDeviceK) return (int)hipErrorInvalidValue;
    if (p.tiles < 1 || p.tiles >= (1LL << 31) || p.m < 1 || p.m >= (1LL << 31) || p.n < 1 || p.n > p.padded || p.padded >= (1LL << 31) / (3 * kMaxDeviceK))
        return (int)hipErrorInvalidValue;
    if ((!p.idx && p.n > p.m) || (p.tile_bytes[0] && !p.out_bytes[0]) || (p.tile_bytes[1] && !p.out_bytes[1])) return (int)hipErrorInvalidValue;
    const long long pieces = (p.padded * 3 * p.K + 3) / 4, work = pieces > p.padded * 3 ? pieces : p.padded * 3;
    const unsigned blocks = (unsigned)((work + 255) / 256 < 4096 ? (work + 255) / 256 : 4096);
    const bool vec = p.K % 4 == 0 && ((reinterpret_cast<uintptr_t>(p.choices) | reinterpret_cast<uintptr_t>(p.out_choices)) & 15) == 0;
    if (vec) hipLaunchKernelGGL(mp_gather_records_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(mp_gather_records_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

int launch_budget_allocate_floor(const AllocateFloorParams& p, void* stream)
{
    if (p.K < 1 || p.K > kMaxDeviceK || p.n < 1 || !p.profile || !p.counts || !p.depth || !p.out_counts || !p.send || !p.totals)
        return (int)hipErrorInvalidValue;
    const long long groups = (p.n + kAllocateWaves - 1) / kAllocateWaves;
    const unsigned blocks = (unsigned)(groups < 4096 ? groups : 4096);
    if (p.emphasis) {
        if (p.tiles < 1) return (int)hipErrorInvalidValue;
        hipLaunchKernelGGL(mp_budget_allocate_floor_kernel<true>, dim3(blocks), dim3(64 * kAllocateWaves), 0, (hipStream_t)stream, p);
    } else hipLaunchKernelGGL(mp_budget_allocate_floor_kernel<false>, dim3(blocks), dim3(64 * kAllocateWaves), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

}  // namespace mpc
