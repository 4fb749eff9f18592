// mp_codes.h -- product: one code of a stream read on the device, with the serial parser's decisions exactly (huffman_step /
// golomb_step of host_bitstream.cpp).  Shared by mp_parse.hip (a lane per chunk, from a checkpoint) and mp_scan.hip (a lane per
// bit position, to find the checkpoints).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mp_device.h"

namespace mpc {
namespace {
// A lane's view of the container: the next `cnt` bits in the top of `buf`, `left` bits to its required end.  After refill() at
// least 33 bits are in the window, so peek() is whole; bits behind the container's end read as zero (the padding) and are never
// consumed: take() refuses what `left` does not cover.
struct Bits {
    const uint32_t* words;
    unsigned long long buf;
    unsigned long long next;            // the next word to load: <= (required end + 63) / 32 + 1, inside the padded buffer
    unsigned long long left;
    unsigned cnt;
    __device__ __forceinline__ void open(const uint32_t* w, unsigned long long begin, unsigned long long end) {
        words = w;
        const unsigned long long word = begin >> 5;
        const unsigned off = (unsigned)(begin & 31u);
        buf = (((unsigned long long)__builtin_bswap32(w[word]) << 32) | __builtin_bswap32(w[word + 1])) << off;
        cnt = 64u - off;
        next = word + 2;
        left = end - begin;
    }
    __device__ __forceinline__ uint32_t peek() const { return (uint32_t)(buf >> 32); }
    __device__ __forceinline__ void refill() {
        if (cnt <= 32u) {
            buf |= (unsigned long long)__builtin_bswap32(words[next]) << (32u - cnt);
            ++next;
            cnt += 32u;
        }
    }
    // k <= 32 bits consumed; false (nothing consumed) = they would pass the required end
    __device__ __forceinline__ bool take(unsigned k) {
        if (k > left) return false;
        buf = k < 64u ? buf << k : 0ull;
        cnt -= k;
        left -= k;
        refill();
        return true;
    }
};

// one Huffman code: 0 = a symbol (*sym), 1 = the pseudo-EOF, 2 = no code here or it would pass the required end
__device__ __forceinline__ int huffman_one(const ParseArgs& a, const ParseStream& st, const uint32_t* lut, Bits& in, unsigned* sym) {
    const uint32_t w = in.peek();
    const uint32_t hit = lut[w >> (32 - kParseLutBits)];            // < kLutSize
    unsigned len = 0, eof = 0, s = 0;
    if (hit != 0u) {
        s = hit & 0xFFFFu;
        len = (hit >> 16) & 63u;
        eof = hit & kParseLutEof;
    } else {
        // longer than the window: the reference's test per length, shortest first.  l <= max_length <= 32: lens holds 33 rows
        for (unsigned l = kParseLutBits + 1; l <= st.max_length; ++l) {
            const uint32_t* row = a.lens + st.len_off + 3u * l;
            const uint32_t count = row[0], first_code = row[1], acc = w >> (32u - l);
            if (count != 0u && acc >= first_code && acc - first_code < count) {
                const uint32_t entry = row[2] + (acc - first_code);  // < total: the host's table (first entry + count <= total)
                eof = entry + 1u == st.total;
                s = a.tables[st.table_off + entry];
                len = l;
                break;
            }
        }
    }
    if (len == 0u || !in.take(len)) return 2;
    *sym = s;
    return eof ? 1 : 0;
}

// one Golomb code (BitBuffer.cpp:228-269); false = it would pass the required end
// kCapped (mp_scan.hip, where a lane stands at every bit and `left` reaches to the container's end): a unary run of
// kScanUnaryCap bits or more is no code either, so a lane takes at most kScanUnaryCap / 32 rounds
template <bool kCapped = false>
__device__ __forceinline__ bool golomb_one(unsigned m, unsigned b, unsigned limit, Bits& in, unsigned* value) {
    unsigned q = 0;
    for (;;) {                                                      // every round consumes bits of `left`: it ends
        const unsigned ones = (unsigned)__clz((int)~in.peek());      // 32 for a window of ones
        if (ones == 32u) {
            if (!in.take(32u)) return false;
            q += 32u;
            if (kCapped && q >= kScanUnaryCap) return false;
            continue;
        }
        if (!in.take(ones + 1u)) return false;                      // the ones and the zero behind them
        q += ones;
        break;
    }
    const unsigned first = b ? in.peek() >> (32u - b) : 0u;         // b <= 16
    if (!in.take(b)) return false;
    unsigned rem = first;
    if (first >= limit) {
        const unsigned bit = in.peek() >> 31;
        if (!in.take(1u)) return false;
        rem = (first << 1) + bit - limit;
    }
    *value = q * m + rem;                                           // 32-bit arithmetic, as on the host; the caller keeps 16 bits
    return true;
}
}  // namespace
}  // namespace mpc
