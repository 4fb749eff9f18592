// host_budget.cpp -- product: the rate control's host definitions (host_budget.h): what mp_budget.hip's allocation kernel computes,
// the rate weights the search of mpc_encode_image_budget takes from the full container's seek index, and for mpc_encode_image_quality
// the allocation's totals at all 256 multipliers (what the sweep kernel computes) and the pick among them.
#include "host_budget.h"

#include "host_bitstream.h"

namespace mpc {

int budget_weights(const uint8_t* index, size_t index_bytes, uint32_t* weights, int* K_out) {
    ContainerIndex x;
    if (!read_container_index(index, index_bytes, x)) return 1;
    const int K = x.K;
    if (K < 1 || K > 32 || x.streams.size() != 1 + 6 * static_cast<size_t>(K)) return 1;
    if (x.serial_only) return 2;
    if (K_out) *K_out = K;
    for (int ch = 0; ch < 3; ++ch)
        for (int i = 0; i < K; ++i) {
            const size_t a = 1 + 2 * static_cast<size_t>(K) * ch + 2 * static_cast<size_t>(i);
            const IndexStream& first = x.streams[a];
            const IndexStream& second = x.streams[a + 1];
            if (second.end_bit < first.wrapper_bit) return 1;
            const uint64_t bits = second.end_bit - first.wrapper_bit, n = first.expect;
            uint64_t w = kBudgetWeightMin;
            if (n != 0) {
                // 256 * bits + n / 2 cannot wrap for any container that fits memory; a blob that says otherwise gets the clamp
                w = bits > (~uint64_t{0} >> 9) ? kBudgetWeightMax : (256 * bits + n / 2) / n;
                if (w < kBudgetWeightMin) w = kBudgetWeightMin;
                if (w > kBudgetWeightMax) w = kBudgetWeightMax;
            }
            if (weights) weights[ch * K + i] = static_cast<uint32_t>(w);
        }
    return 0;
}

void budget_allocate(const uint32_t* profile, const uint16_t* counts, long long tiles, int K, const uint32_t* weights, int j, uint8_t* depth,
                     uint16_t* out_counts, uint64_t totals[3]) {
    budget_allocate_emphasis(profile, counts, nullptr, tiles, K, weights, j, depth, out_counts, totals);
}

void budget_allocate_emphasis(const uint32_t* profile, const uint16_t* counts, const uint8_t* emphasis, long long tiles, int K,
                              const uint32_t* weights, int j, uint8_t* depth, uint16_t* out_counts, uint64_t totals[3]) {
    const uint64_t L = budget_lambda(j);
    uint32_t below[3][33];                              // below[ch][m] = W[ch][0] + ... + W[ch][m - 1]
    for (int ch = 0; ch < 3; ++ch) {
        below[ch][0] = 0;
        for (int i = 0; i < K; ++i) below[ch][i + 1] = below[ch][i] + weights[ch * K + i];
    }
    totals[0] = totals[1] = totals[2] = 0;
    for (long long t = 0; t < tiles; ++t) {
        int cnt[3];
        for (int ch = 0; ch < 3; ++ch) cnt[ch] = counts[t * 3 + ch] > K ? K : counts[t * 3 + ch];
        const uint32_t* P = profile + t * (K + 1);
        const uint64_t factor = static_cast<uint64_t>(emphasis ? emphasis_used(emphasis[t]) : kEmphasisNeutral) << kEmphasisShift;
        uint64_t best = 0, best_rate = 0;
        int at = 0;
        for (int n = 0; n <= K; ++n) {
            uint64_t rate = 0;
            for (int ch = 0; ch < 3; ++ch) rate += below[ch][n < cnt[ch] ? n : cnt[ch]];
            const uint64_t J = P[n] * factor + L * rate;
            if (n == 0 || J < best) {
                best = J;
                best_rate = rate;
                at = n;
            }
        }
        if (depth) depth[t] = static_cast<uint8_t>(at);
        totals[0] += P[at];
        totals[1] += best_rate;
        for (int ch = 0; ch < 3; ++ch) {
            const int kept = at < cnt[ch] ? at : cnt[ch];
            if (out_counts) out_counts[t * 3 + ch] = static_cast<uint16_t>(kept);
            totals[2] += static_cast<uint64_t>(kept);
        }
    }
}

void budget_sweep(const uint32_t* profile, const uint16_t* counts, long long tiles, int K, const uint32_t* weights, uint64_t totals[3 * kBudgetLambdas]) {
    budget_sweep_emphasis(profile, counts, nullptr, tiles, K, weights, totals);
}

void budget_sweep_emphasis(const uint32_t* profile, const uint16_t* counts, const uint8_t* emphasis, long long tiles, int K,
                           const uint32_t* weights, uint64_t totals[3 * kBudgetLambdas]) {
    uint64_t L[kBudgetLambdas];
    for (int j = 0; j < kBudgetLambdas; ++j) {
        L[j] = budget_lambda(j);
        totals[3 * j] = totals[3 * j + 1] = totals[3 * j + 2] = 0;
    }
    uint32_t below[3][33];                              // below[ch][m] = W[ch][0] + ... + W[ch][m - 1]
    for (int ch = 0; ch < 3; ++ch) {
        below[ch][0] = 0;
        for (int i = 0; i < K; ++i) below[ch][i + 1] = below[ch][i] + weights[ch * K + i];
    }
    for (long long t = 0; t < tiles; ++t) {
        // the tile's own: distortion term, rate and records kept of every depth, once for all multipliers
        const uint64_t factor = static_cast<uint64_t>(emphasis ? emphasis_used(emphasis[t]) : kEmphasisNeutral) << kEmphasisShift;
        uint64_t scaled[33], rate[33], kept[33];
        for (int n = 0; n <= K; ++n) {
            scaled[n] = profile[t * (K + 1) + n] * factor;
            rate[n] = kept[n] = 0;
            for (int ch = 0; ch < 3; ++ch) {
                const int count = counts[t * 3 + ch] > K ? K : counts[t * 3 + ch];
                const int upto = n < count ? n : count;
                rate[n] += below[ch][upto];
                kept[n] += static_cast<uint64_t>(upto);
            }
        }
        for (int j = 0; j < kBudgetLambdas; ++j) {
            int at = 0;
            uint64_t best = scaled[0] + L[j] * rate[0];
            for (int n = 1; n <= K; ++n) {
                const uint64_t J = scaled[n] + L[j] * rate[n];
                if (J < best) {                         // the first strict minimum: the smallest n wins ties
                    best = J;
                    at = n;
                }
            }
            totals[3 * j] += profile[t * (K + 1) + at];
            totals[3 * j + 1] += rate[at];
            totals[3 * j + 2] += kept[at];
        }
    }
}

void emphasis_from_mask(const uint8_t* mask, int width, int height, size_t row_stride, int lo, int hi, uint8_t* emphasis) {
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    for (int tx = 0; tx < tiles_x; ++tx)
        for (int ty = 0; ty < tiles_y; ++ty) {
            const int x_end = tx * 8 + 8 < width ? tx * 8 + 8 : width, y_end = ty * 8 + 8 < height ? ty * 8 + 8 : height;
            int m = 0;
            for (int y = ty * 8; y < y_end; ++y)
                for (int x = tx * 8; x < x_end; ++x) {
                    const int v = mask[static_cast<size_t>(y) * row_stride + static_cast<size_t>(x)];
                    m = v > m ? v : m;
                }
            emphasis[static_cast<size_t>(tx) * tiles_y + ty] = static_cast<uint8_t>(lo + ((hi - lo) * m + 127) / 255);
        }
}

void budget_allocate_group(const uint32_t* profile, const uint16_t* counts, const uint8_t* emphasis, int frames, long long tiles, int K,
                           const uint32_t* weights, int j, uint8_t* depth, uint16_t* out_counts, uint64_t* totals) {
    const uint64_t L = budget_lambda(j);
    const long long all = static_cast<long long>(frames) * tiles;
    for (int k = 0; k < 3 * frames; ++k) totals[k] = 0;
    uint32_t below[3][33];                              // the frame's at hand: below[ch][m] = W[f][ch][0] + ... + W[f][ch][m - 1]
    int built_for = -1;
    for (long long g = 0; g < all; ++g) {               // one walk over the tiles of the whole group, frame-major
        const int f = static_cast<int>(g / tiles);
        if (f != built_for) {
            const uint32_t* W = weights + static_cast<size_t>(f) * 3 * K;
            for (int ch = 0; ch < 3; ++ch) {
                below[ch][0] = 0;
                for (int i = 0; i < K; ++i) below[ch][i + 1] = below[ch][i] + W[ch * K + i];
            }
            built_for = f;
        }
        const uint32_t* P = profile + g * (K + 1);
        const uint64_t factor = static_cast<uint64_t>(emphasis ? emphasis_used(emphasis[g]) : kEmphasisNeutral) << kEmphasisShift;
        int cnt[3], at = 0;
        uint64_t rate_at[33];
        uint64_t best = 0;
        for (int ch = 0; ch < 3; ++ch) cnt[ch] = counts[g * 3 + ch] > K ? K : counts[g * 3 + ch];
        for (int n = 0; n <= K; ++n) {
            rate_at[n] = 0;
            for (int ch = 0; ch < 3; ++ch) rate_at[n] += below[ch][n < cnt[ch] ? n : cnt[ch]];
            const uint64_t J = P[n] * factor + L * rate_at[n];
            if (n == 0 || J < best) {                   // the first strict minimum: the smallest n wins ties
                best = J;
                at = n;
            }
        }
        if (depth) depth[g] = static_cast<uint8_t>(at);
        uint64_t* mine = totals + 3 * static_cast<size_t>(f);
        mine[0] += P[at];
        mine[1] += rate_at[at];
        for (int ch = 0; ch < 3; ++ch) {
            const int kept = at < cnt[ch] ? at : cnt[ch];
            if (out_counts) out_counts[g * 3 + ch] = static_cast<uint16_t>(kept);
            mine[2] += static_cast<uint64_t>(kept);
        }
    }
}

void budget_sweep_group(const uint32_t* profile, const uint16_t* counts, const uint8_t* emphasis, int frames, long long tiles, int K,
                        const uint32_t* weights, uint64_t totals[3 * kBudgetLambdas]) {
    for (int k = 0; k < 3 * kBudgetLambdas; ++k) totals[k] = 0;
    for (int f = 0; f < frames; ++f) {
        const uint32_t* W = weights + static_cast<size_t>(f) * 3 * K;
        uint32_t below[3][33];                          // frame f's: below[ch][m] = W[ch][0] + ... + W[ch][m - 1]
        for (int ch = 0; ch < 3; ++ch) {
            below[ch][0] = 0;
            for (int i = 0; i < K; ++i) below[ch][i + 1] = below[ch][i] + W[ch * K + i];
        }
        for (long long t = 0; t < tiles; ++t) {
            const long long g = static_cast<long long>(f) * tiles + t;
            const uint64_t factor = static_cast<uint64_t>(emphasis ? emphasis_used(emphasis[g]) : kEmphasisNeutral) << kEmphasisShift;
            uint64_t scaled[33], rate[33], kept[33];
            for (int n = 0; n <= K; ++n) {
                scaled[n] = profile[g * (K + 1) + n] * factor;
                rate[n] = kept[n] = 0;
                for (int ch = 0; ch < 3; ++ch) {
                    const int count = counts[g * 3 + ch] > K ? K : counts[g * 3 + ch];
                    const int upto = n < count ? n : count;
                    rate[n] += below[ch][upto];
                    kept[n] += static_cast<uint64_t>(upto);
                }
            }
            // the ladder downwards: L falls, so the walk over n is the same first strict minimum at every j
            for (int j = kBudgetLambdas - 1; j >= 0; --j) {
                const uint64_t L = budget_lambda(j);
                int at = 0;
                uint64_t best = scaled[0] + L * rate[0];
                for (int n = 1; n <= K; ++n) {
                    const uint64_t J = scaled[n] + L * rate[n];
                    if (J < best) {
                        best = J;
                        at = n;
                    }
                }
                totals[3 * j] += profile[g * (K + 1) + at];
                totals[3 * j + 1] += rate[at];
                totals[3 * j + 2] += kept[at];
            }
        }
    }
}

int quality_pick(const uint64_t totals[3 * kBudgetLambdas], uint64_t max_sse) {
    for (int j = kBudgetLambdas - 1; j >= 0; --j)
        if (totals[3 * j] <= max_sse) return j;
    return -1;
}

}  // namespace mpc
