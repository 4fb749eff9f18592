// host_rate.cpp -- product: the host definitions of a delta stream to a byte budget (host_rate.h): what mp_rate.hip's owed-flags and
// floor allocation kernels compute.
#include "host_rate.h"

#include "host_budget.h"

namespace mpc {

long long owed_tiles(const uint8_t* sent, const uint16_t* counts, long long tiles, int K, const int32_t* changed, long long n_changed,
                     int32_t* candidates, uint8_t* floor, uint8_t* must) {
    long long n = 0, next = 0;                          // `changed` ascends: one walk beside the tiles
    for (long long t = 0; t < tiles; ++t) {
        const bool is_changed = next < n_changed && changed[next] == t;
        if (is_changed) ++next;
        int full = 0;
        for (int ch = 0; ch < 3; ++ch) {
            const int count = counts[t * 3 + ch] > K ? K : counts[t * 3 + ch];
            full = count > full ? count : full;
        }
        if (must) must[t] = is_changed ? 1 : 0;
        if (floor) floor[t] = is_changed ? 0 : sent[t];
        if (is_changed || sent[t] < full) {
            if (candidates) candidates[n] = static_cast<int32_t>(t);
            ++n;
        }
    }
    return n;
}

void budget_allocate_floor(const uint32_t* profile, const uint16_t* counts, const uint8_t* floor, const uint8_t* must, long long n, int K,
                           const uint32_t* weights, int j, uint8_t* depth, uint16_t* out_counts, uint8_t* send, uint64_t totals[4]) {
    budget_allocate_floor_emphasis(profile, counts, floor, must, nullptr, nullptr, 0, n, K, weights, j, depth, out_counts, send, totals);
}

void budget_allocate_floor_emphasis(const uint32_t* profile, const uint16_t* counts, const uint8_t* floor, const uint8_t* must,
                                    const uint8_t* emphasis, const int32_t* list, long long tiles, long long n, int K, const uint32_t* weights,
                                    int j, uint8_t* depth, uint16_t* out_counts, uint8_t* send, uint64_t totals[4]) {
    const uint64_t L = budget_lambda(j);
    uint32_t below[3][33];                              // below[ch][m] = W[ch][0] + ... + W[ch][m - 1]
    for (int ch = 0; ch < 3; ++ch) {
        below[ch][0] = 0;
        for (int i = 0; i < K; ++i) below[ch][i + 1] = below[ch][i] + weights[ch * K + i];
    }
    totals[0] = totals[1] = totals[2] = totals[3] = 0;
    for (long long i = 0; i < n; ++i) {
        int cnt[3];
        for (int ch = 0; ch < 3; ++ch) cnt[ch] = counts[i * 3 + ch] > K ? K : counts[i * 3 + ch];
        const bool has_to = must ? must[i] != 0 : true;
        const int low = floor ? (floor[i] > K ? K : floor[i]) : 0;
        const uint32_t* P = profile + i * (K + 1);
        const long long t = list ? static_cast<long long>(list[i]) : i;
        const uint64_t factor = static_cast<uint64_t>(emphasis && t >= 0 && t < tiles ? emphasis_used(emphasis[t]) : kEmphasisNeutral) << kEmphasisShift;
        uint64_t best = 0, best_rate = 0;
        int at = -1;
        for (int d = has_to ? 0 : low; d <= K; ++d) {
            uint64_t rate = 0;
            if (has_to || d != low)
                for (int ch = 0; ch < 3; ++ch) rate += below[ch][d < cnt[ch] ? d : cnt[ch]];
            const uint64_t J = P[d] * factor + L * rate;
            if (at < 0 || J < best) {
                best = J;
                best_rate = rate;
                at = d;
            }
        }
        const bool sends = has_to || at > low;
        if (depth) depth[i] = static_cast<uint8_t>(at);
        if (send) send[i] = sends ? 1 : 0;
        totals[0] += P[at];
        totals[1] += best_rate;
        totals[3] += sends ? 1 : 0;
        for (int ch = 0; ch < 3; ++ch) {
            const int kept = at < cnt[ch] ? at : cnt[ch];
            if (out_counts) out_counts[i * 3 + ch] = static_cast<uint16_t>(kept);
            if (sends) totals[2] += static_cast<uint64_t>(kept);
        }
    }
}

}  // namespace mpc
