// mp_scan.hip -- product: the seek index's checkpoints found on the device, without walking a stream's codes one after another:
// what the host's HostStreamScanner (host_container.cpp) is to mpc_container_index_scan.
//
// Which code begins at bit p of a stream, and how long it is, is a function of the bits at p and the stream's table alone
// (huffman_one / golomb_one of mp_codes.h, the serial parser's step).  Evaluated at every bit of a window, the serial parse is the
// walk p -> p + len(p) from the stream's first code, and that walk composes: per segment, per super-segment of kScanSuper
// segments, and along the window.  Nothing waits for a code to re-synchronise, so uniform codes (which never do) cost the same.
//
//   step      a lane per bit position: the code the serial parser's step finds there -- its length, or the pseudo-EOF and its
//             length, or "no code here, or it would pass the container's end".  The table in LDS as mp_parse_kernel keeps it; a
//             lane's two or three words are its neighbours' words, so the loads coalesce.
//   segment   a lane per segment, right to left: exit[p] = the first code start at or behind the segment's end on the path from p
//             (a long Golomb code jumps over whole segments), count[p] = the codes on that path.  Terminal: the bit behind the
//             pseudo-EOF, or dead -- count is then the codes before the path ends.
//   super     a lane per bit of a super-segment's first segment: exit and count over the super-segment's kScanSuper segments.
//   chain     one wave.  Lane 0 walks from the window's first bit: a super-segment it enters in its first segment and whose path
//             neither ends nor reaches the stream's n-th code is taken in one look-up, anything else segment by segment; then the
//             lanes, a super-segment each, write the entry and first ordinal of every segment the walk jumped.
//   emit      a lane per segment: from its true entry and first ordinal it walks its own piece of the chain and writes the bit of
//             every code whose ordinal is a multiple of `interval`; the lane of the last segment writes where the stream ends.
//
// The input is untrusted.  Why every loop ends, and inside what every address lies (ScanArgs's sizes are the host's: the window,
// the segment count, the container's padded size; none is a decoded value):
//   step      one code per lane.  Huffman: at most 32 - kParseLutBits per-length tests.  Golomb: a round per 32 bits of the unary
//             run, at most kScanUnaryCap / 32 of them (golomb_one<true>), each inside `left` = total_bits - p.  Reads: words up to
//             (total_bits + 63) / 32 + 1, inside the 16 bytes of zero padding.  Writes: step[p], p < win_bits.
//   segment   seg_bits rounds at most; reads step[p], exit_of[next], count[next] with p < next < the segment's end <= win_bits.
//             The LDS form (segments of at most 256 bits): the same pass on rows of 257 words, indexed by a bit's offset in its
//             segment (< seg_bits <= 256) and the segment's row in the workgroup (< 16); global reads and writes at
//             lo0 + i < win_bits.
//   super     kScanSuper rounds at most: every round leaves a segment through its exit, which lies at or behind that segment's end;
//             exit_of is read at positions < win_bits only.
//   chain     lane 0: n_segs + 1 rounds at most, every round enters a later segment or stops; the lanes: kScanSuper rounds per
//             super-segment, n_supers / 64 super-segments each.
//   emit      seg_bits + 1 rounds at most: every code takes a bit at least, so at most seg_bits codes begin in a segment.  A
//             checkpoint is written at ordinal / interval only for ordinal < n, so inside the stream's n_cp entries.
// No kernel iterates until nothing changes.  A damaged container yields dead chains, miscounts and give-ups; the host then asks
// the serial builder, whose verdict is the caller's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mp_device.h"
#include "mp_codes.h"

namespace mpc {

namespace {
constexpr int kLutSize = 1 << kParseLutBits;
constexpr int kStepBlock = 256;
constexpr unsigned kSegLds = 256, kSegRows = 16;
}  // namespace

__global__ __launch_bounds__(256) void mp_scan_step_kernel(const ScanArgs a)
{
    __shared__ uint32_t lut[kLutSize];
    const ParseStream& st = a.stream;
    const bool golomb = (st.flags & kParseGolomb) != 0u;
    if (!golomb) {
        const uint4* src = reinterpret_cast<const uint4*>(a.tables.luts);        // one whole table: the host uploads it per stream
        for (int i = threadIdx.x; i < kLutSize / 4; i += kStepBlock) reinterpret_cast<uint4*>(lut)[i] = src[i];
    }
    __syncthreads();
    const unsigned p = blockIdx.x * kStepBlock + threadIdx.x;
    if (p >= a.win_bits) return;
    Bits in;
    in.open(a.tables.words, a.win_begin + p, a.total_bits);                      // win_begin + p < total_bits
    const unsigned long long before = in.left;
    unsigned value = 0, word = kScanStepDead;
    if (golomb) {
        const unsigned b = 32u - (unsigned)__clz((int)st.m);                     // bit_width(M), M >= 1
        const unsigned limit = (1u << (b + 1u)) - st.m;
        if (golomb_one<true>(st.m, b, limit, in, &value)) word = (unsigned)(before - in.left);
    } else {
        const int what = huffman_one(a.tables, st, lut, in, &value);
        if (what != 2) word = (unsigned)(before - in.left) | (what == 1 ? kScanStepEof : 0u);
    }
    a.step[p] = word;
}

__global__ __launch_bounds__(64) void mp_scan_segment_kernel(const ScanArgs a)
{
    const unsigned seg = blockIdx.x * 64 + threadIdx.x;
    if (seg >= a.n_segs) return;
    const unsigned lo = seg * a.seg_bits;                                        // < win_bits: n_segs = ceil(win_bits / seg_bits)
    const unsigned hi = lo + a.seg_bits < a.win_bits ? lo + a.seg_bits : a.win_bits;
    for (unsigned p = hi; p-- > lo;) {
        const unsigned s = a.step[p], next = p + (s & kScanStepLen);
        unsigned e, c;
        if (s & kScanStepDead) { e = kScanExitDead; c = 0u; }
        else if (s & kScanStepEof) { e = kScanExitEof | next; c = 0u; }
        else if (next >= hi) { e = next; c = 1u; }
        else { e = a.exit_of[next]; c = a.count[next] + 1u; }                    // p < next < hi: this lane wrote it
        a.exit_of[p] = e;
        a.count[p] = (uint16_t)c;                                                // <= hi - p <= seg_bits <= 32768
    }
}

// The same for segments of at most kSegLds bits (the default's 256), sixteen segments a workgroup: the right-to-left pass is a chain
// of dependent reads, a few hundred of them, so the steps come in and the maps go out as coalesced words and the chain itself runs
// in LDS.  Rows are padded by a word: the sixteen lanes of the pass stand a whole row apart.
__global__ __launch_bounds__(256) void mp_scan_segment_lds_kernel(const ScanArgs a)
{
    __shared__ unsigned s_step[kSegRows * (kSegLds + 1)];
    __shared__ unsigned s_exit[kSegRows * (kSegLds + 1)];
    __shared__ uint16_t s_count[kSegRows * (kSegLds + 2)];
    const unsigned S = a.seg_bits;                                               // <= kSegLds: the launcher's choice
    const unsigned seg0 = blockIdx.x * kSegRows;                                 // < n_segs: the grid
    const unsigned lo0 = seg0 * S;                                               // < win_bits
    const unsigned span = kSegRows * S < a.win_bits - lo0 ? kSegRows * S : a.win_bits - lo0;
    for (unsigned i = threadIdx.x; i < span; i += 256) {
        const unsigned r = i / S, o = i - r * S;                                 // r < kSegRows, o < S
        s_step[r * (kSegLds + 1) + o] = a.step[lo0 + i];
    }
    __syncthreads();
    const unsigned seg = seg0 + threadIdx.x;
    if (threadIdx.x < kSegRows && seg < a.n_segs) {
        const unsigned r = threadIdx.x, lo = seg * S;
        const unsigned n = lo + S < a.win_bits ? S : a.win_bits - lo;            // the segment's bits
        for (unsigned o = n; o-- > 0;) {
            const unsigned s = s_step[r * (kSegLds + 1) + o], next = o + (s & kScanStepLen);
            unsigned e, c;
            if (s & kScanStepDead) { e = kScanExitDead; c = 0u; }
            else if (s & kScanStepEof) { e = kScanExitEof | (lo + next); c = 0u; }
            else if (next >= n) { e = lo + next; c = 1u; }
            else { e = s_exit[r * (kSegLds + 1) + next]; c = s_count[r * (kSegLds + 2) + next] + 1u; }      // o < next < n
            s_exit[r * (kSegLds + 1) + o] = e;
            s_count[r * (kSegLds + 2) + o] = (uint16_t)c;
        }
    }
    __syncthreads();
    for (unsigned i = threadIdx.x; i < span; i += 256) {
        const unsigned r = i / S, o = i - r * S;
        a.exit_of[lo0 + i] = s_exit[r * (kSegLds + 1) + o];
        a.count[lo0 + i] = s_count[r * (kSegLds + 2) + o];
    }
}

__global__ __launch_bounds__(256) void mp_scan_super_kernel(const ScanArgs a)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (unsigned long long)a.n_supers * a.seg_bits) return;
    const unsigned sup = (unsigned)(i / a.seg_bits), off = (unsigned)(i - (unsigned long long)sup * a.seg_bits);
    const unsigned long long span = (unsigned long long)kScanSuper * a.seg_bits;
    const unsigned long long end64 = (sup + 1ull) * span;
    const unsigned end = end64 < a.win_bits ? (unsigned)end64 : a.win_bits;
    unsigned pos = (unsigned)(sup * span) + off;                                 // sup * span < win_bits
    unsigned e = kScanExitDead, c = 0u;
    if (pos < end) {
        e = pos;
        for (unsigned k = 0; k < kScanSuper && e < end; ++k) {                   // e: a plain position here
            const unsigned x = a.exit_of[e];                                     // e < end <= win_bits
            c += a.count[e];
            e = x;
            if (x & (kScanExitDead | kScanExitEof)) break;
        }
        if (!(e & (kScanExitDead | kScanExitEof)) && e < end) e = kScanExitDead; // cannot be: every round leaves a segment
    }
    a.sup_exit[i] = e;
    a.sup_count[i] = c;
}

__global__ __launch_bounds__(64) void mp_scan_chain_kernel(const ScanArgs a)
{
    const int lane = threadIdx.x;
    const bool golomb = (a.stream.flags & kParseGolomb) != 0u;
    for (unsigned s = lane; s < a.n_segs; s += 64) a.seg_entry[s] = kScanNoEntry;
    for (unsigned s = lane; s < a.n_supers; s += 64) a.sup_entry[s] = kScanNoEntry;
    __syncthreads();
    if (lane == 0) {
        unsigned long long pos = 0, ord = a.ord0;
        ScanResult r;
        r.state = kScanContinue;
        r.final_seg = kScanNoEntry;
        for (unsigned it = 0; it <= a.n_segs && pos < a.win_bits; ++it) {
            const unsigned p = (unsigned)pos, seg = p / a.seg_bits, sup = seg / kScanSuper;
            if (seg % kScanSuper == 0u) {                                        // a whole super-segment in one look-up?
                const unsigned long long i = (unsigned long long)sup * a.seg_bits + (p - seg * a.seg_bits);
                const unsigned e = a.sup_exit[i], c = a.sup_count[i];
                if (!(e & (kScanExitDead | kScanExitEof)) && (!golomb || ord + c < a.n)) {
                    a.sup_entry[sup] = p;
                    a.sup_ord[sup] = ord;
                    pos = e;
                    ord += c;
                    continue;
                }
            }
            const unsigned e = a.exit_of[p], c = a.count[p];
            // a Golomb stream ends behind its n-th code, whatever the path behind that runs into
            const bool ends_here = (e & kScanExitEof) || (golomb && ord + c >= a.n);
            if ((e & kScanExitDead) && !ends_here) {
                r.state = kScanDead;
                break;
            }
            a.seg_entry[seg] = p;
            a.seg_ord[seg] = ord;
            if (ends_here) {
                r.state = 0u;                                                    // the emit kernel's lane of this segment says how
                r.final_seg = seg;
                break;
            }
            pos = e & kScanExitPos;
            ord += c;
        }
        r.position = a.win_begin + pos;
        r.ordinal = ord;
        *a.result = r;
    }
    __syncthreads();
    for (unsigned sup = lane; sup < a.n_supers; sup += 64) {
        unsigned p = a.sup_entry[sup];
        if (p == kScanNoEntry) continue;
        unsigned long long ord = a.sup_ord[sup];
        const unsigned long long end64 = (sup + 1ull) * kScanSuper * a.seg_bits;
        const unsigned end = end64 < a.win_bits ? (unsigned)end64 : a.win_bits;
        for (unsigned k = 0; k < kScanSuper && p < end; ++k) {
            const unsigned seg = p / a.seg_bits;                                 // p < win_bits: seg < n_segs
            a.seg_entry[seg] = p;
            a.seg_ord[seg] = ord;
            const unsigned e = a.exit_of[p];
            ord += a.count[p];
            if (e & (kScanExitDead | kScanExitEof)) break;                       // cannot be: the super-segment's path was plain
            p = e;
        }
    }
}

__global__ __launch_bounds__(64) void mp_scan_emit_kernel(const ScanArgs a)
{
    const unsigned seg = blockIdx.x * 64 + threadIdx.x;
    if (seg >= a.n_segs) return;
    unsigned p = a.seg_entry[seg];
    if (p == kScanNoEntry) return;
    const bool golomb = (a.stream.flags & kParseGolomb) != 0u;
    const bool final_seg = a.result->final_seg == seg;
    const unsigned hi = (seg + 1u) * a.seg_bits < a.win_bits ? (seg + 1u) * a.seg_bits : a.win_bits;     // p < hi: an entry lies in its segment
    unsigned long long q = a.seg_ord[seg];
    unsigned state = kScanDead;                                                  // the last segment's walk must end the stream
    unsigned long long end = 0;
    for (unsigned k = 0; k <= a.seg_bits; ++k) {
        if (golomb && q == a.n) {
            state = kScanEnded;
            end = a.win_begin + p;
            break;
        }
        if (p >= hi) break;
        if (q < a.n && q % a.interval == 0u) a.checkpoints[q / a.interval] = a.win_begin + p;            // q / interval < n_cp
        const unsigned s = a.step[p];
        if (s & kScanStepDead) break;
        if (s & kScanStepEof) {
            state = q == a.n ? kScanEnded : kScanMiscount;
            end = a.win_begin + p + (s & kScanStepLen);
            break;
        }
        p += s & kScanStepLen;
        ++q;
    }
    if (final_seg) {
        a.result->state = state;
        a.result->position = end;
        a.result->ordinal = q;
    }
}

namespace {
bool scan_args_ok(const ScanArgs& a) {
    if (a.seg_bits < 32u || a.seg_bits > 32768u || a.win_bits < 1u || a.win_bits > (1u << 26) || a.interval < 1u) return false;
    if (a.win_begin >= a.total_bits || a.win_bits > a.total_bits - a.win_begin) return false;
    if (a.n_segs != (a.win_bits + a.seg_bits - 1u) / a.seg_bits || a.n_supers != (a.n_segs + kScanSuper - 1u) / kScanSuper) return false;
    if (a.n_cp != (a.n + a.interval - 1u) / a.interval) return false;
    if ((a.stream.flags & kParseGolomb) ? a.stream.m == 0u : (a.stream.max_length > 32u || a.stream.total == 0u)) return false;
    return a.step && a.exit_of && a.count && a.sup_exit && a.sup_count && a.sup_entry && a.sup_ord && a.seg_entry && a.seg_ord &&
           a.checkpoints && a.result && a.tables.words;
}
}  // namespace

int launch_scan_window(const ScanArgs& a, void* stream_)
{
    if (!scan_args_ok(a)) return (int)hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(mp_scan_step_kernel, dim3((a.win_bits + kStepBlock - 1) / kStepBlock), dim3(kStepBlock), 0, s, a);
    if (a.seg_bits <= kSegLds) hipLaunchKernelGGL(mp_scan_segment_lds_kernel, dim3((a.n_segs + kSegRows - 1) / kSegRows), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(mp_scan_segment_kernel, dim3((a.n_segs + 63) / 64), dim3(64), 0, s, a);
    const unsigned long long sup_lanes = (unsigned long long)a.n_supers * a.seg_bits;
    hipLaunchKernelGGL(mp_scan_super_kernel, dim3((unsigned)((sup_lanes + 255) / 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(mp_scan_chain_kernel, dim3(1), dim3(64), 0, s, a);
    hipLaunchKernelGGL(mp_scan_emit_kernel, dim3((a.n_segs + 63) / 64), dim3(64), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace mpc
