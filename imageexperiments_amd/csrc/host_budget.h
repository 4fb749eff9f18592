// host_budget.h -- product: the host's definition of the rate control behind mpc_encode_image_budget (include/mpcodec.h, "budget";
// DESIGN.md 4, "Encoder: a byte budget"): the multiplier table, the rate weights from a seek index, the allocation at one multiplier;
// and behind mpc_encode_image_quality ("quality"): the allocation's totals at every multiplier, the pick, the squared error of a PSNR.
// And the emphasis map ("emphasis"; DESIGN.md 4, "Encoder: emphasis"): a factor per tile on the distortion term of both, and the map from
// a pixel mask.  Knows neither HIP nor the C ABI and builds on its own with host_bitstream / host_container (tests/cpp/asan_budget.cpp,
// asan_quality.cpp, asan_emphasis.cpp, asan_group.cpp).
#pragma once

#include <cstddef>
#include <cstdint>

namespace mpc {

constexpr int kBudgetLambdas = 256;                 // multipliers j = 0 ... 255
constexpr uint32_t kBudgetWeightMin = 256;          // one bit, in 1/256 bit
constexpr uint32_t kBudgetWeightMax = 1u << 20;     // 4096 bits
constexpr int kBudgetDistortionShift = 16;          // J = P * 65536 + L * R

// L[0] = 0, L[j] = (8 + (j - 1) % 8) << ((j - 1) / 8): a geometric grid, eight values an octave (steps of 12.5 % down to 6.7 %).
// L[255] = 14 << 31.  A record weighs at least 256 (one bit), so keeping any record costs at least 14 * 2^39 > 2^42, while a tile's
// largest possible distortion term is 64 * 3 * 255^2 * 65536 < 2^40: at j = 255 every depth is 0.
inline uint64_t budget_lambda(int j) { return j <= 0 ? 0 : static_cast<uint64_t>(8 + (j - 1) % 8) << ((j - 1) / 8); }

// W[ch][i] at weights[ch * K + i], K the index's, from a seek index (either version) of the frame's full container: with
// a = 1 + 2K * ch + 2i, bits = end_bit(a + 1) - wrapper_bit(a), n = expect(a): clamp((256 * bits + n / 2) / n, 256, 2^20), 256 when
// n = 0.  Returns 0; 1 = not a seek index (or one whose streams do not lie one behind the other); 2 = a serial-only index.
// weights == nullptr: the verdict alone.  *K_out (optional): the index's K
int budget_weights(const uint8_t* index, size_t index_bytes, uint32_t* weights, int* K_out = nullptr);

// The allocation at multiplier j over `tiles` tiles: profile[t * (K + 1) + n], counts[t * 3 + ch] (a count above K is used as K),
// weights[ch * K + i].  R(t, n) = sum over ch, i < min(n, count) of W[ch][i]; J(t, n) = P * 65536 + L[j] * R in u64; depth[t] = the
// smallest n of 0 ... K that minimises J; out_counts = min(count, depth[t]); totals[0] = sum P[t][depth], [1] = sum R[t][depth],
// [2] = the records kept.  depth, out_counts: each may be null.  The caller has checked: 1 <= K <= 32, 0 <= j < 256, tiles >= 0
void budget_allocate(const uint32_t* profile, const uint16_t* counts, long long tiles, int K, const uint32_t* weights, int j, uint8_t* depth,
                     uint16_t* out_counts, uint64_t totals[3]);

// ---- encode to a target quality (include/mpcodec.h, "quality"; DESIGN.md 4, "Encoder: a target quality") ----
// The sweep: totals[3 * j + k], j = 0 ... 255, k = 0 ... 2 = what budget_allocate's totals[k] are at multiplier j for the same profile,
// counts and weights.  It defines what mp_budget_sweep_kernel computes.  A loop of its own over tiles and multipliers that works out a
// tile's rates once -- not 256 calls of budget_allocate, so that the two check each other.  The caller has checked what budget_allocate's has
void budget_sweep(const uint32_t* profile, const uint16_t* counts, long long tiles, int K, const uint32_t* weights, uint64_t totals[3 * kBudgetLambdas]);

// The pick: the largest j with totals[3 * j] <= max_sse, -1 if there is none.  The distortion total does not fall along the ladder
// (L[j] rises strictly, so a tile's P at its minimiser cannot fall), which makes this the boundary a bisection would find; it is
// defined, and computed, as the largest j
int quality_pick(const uint64_t totals[3 * kBudgetLambdas], uint64_t max_sse);

// The largest s in 0 ... limit with psnr(s) >= target, psnr a function that does not rise with s and is +inf at 0 (psnr_from_sse of
// host_codec.h at one geometry): a binary search on that very function, so the answer agrees with it to the bit.  target: not NaN
// ---- emphasis maps (include/mpcodec.h, "emphasis"; DESIGN.md 4, "Encoder: emphasis") ----
// e[t], one u8 per tile, four fractional bits: 16 is neutral, the range 1 ... 64; a stored 0 is used as 1 and a value above 64 as 64 (no
// address ever comes from one).  J(t, n) = P * e[t] * 4096 + L[j] * R: with e = 16 the factor is 65536 and J is budget_allocate's.
// P <= 64 * 3 * 255^2 = 12 484 800, so P * 64 * 4096 <= 3.28e12 < 14 * 2^39 = 7.70e12, the cost of the cheapest record at j = 255: there
// every depth is still 0, the budget search keeps its feasible end, and J stays below 2^63.
constexpr int kEmphasisNeutral = 16;
constexpr int kEmphasisMax = 64;
constexpr int kEmphasisShift = 12;                  // e * 4096: 16 * 4096 = 1 << kBudgetDistortionShift
static_assert((kEmphasisNeutral << kEmphasisShift) == (1 << kBudgetDistortionShift), "the neutral value is the plain allocation");
constexpr uint32_t emphasis_used(uint8_t stored) {  // constexpr: the kernels use it too
    return stored == 0 ? 1u : stored > kEmphasisMax ? static_cast<uint32_t>(kEmphasisMax) : stored;
}

// budget_allocate with J(t, n) = P[t][n] * e[t] * 4096 + L[j] * R[t][n]; totals[0] stays the sum of the unweighted P[t][depth[t]], the
// squared error a decoder shows.  emphasis[tiles], null = neutral: then budget_allocate itself, bit for bit
void budget_allocate_emphasis(const uint32_t* profile, const uint16_t* counts, const uint8_t* emphasis, long long tiles, int K,
                              const uint32_t* weights, int j, uint8_t* depth, uint16_t* out_counts, uint64_t totals[3]);
// budget_sweep with the same J: totals[3 * j + k] = budget_allocate_emphasis's totals[k] at multiplier j.  A loop of its own, as
// budget_sweep is.  Scaling a tile's P by a positive constant leaves the argument of quality_pick intact: a tile's P at its minimiser
// does not fall as L rises, so totals[3 * j], the true squared error, still never falls along the ladder
void budget_sweep_emphasis(const uint32_t* profile, const uint16_t* counts, const uint8_t* emphasis, long long tiles, int K,
                           const uint32_t* weights, uint64_t totals[3 * kBudgetLambdas]);
// mask[y * row_stride + x], x < width, y < height (row_stride >= width; the bytes between rows are never read) -> emphasis[t],
// t = tx * tiles_y + ty over the 8 x 8 tiles: lo + ((hi - lo) * m + 127) / 255, m the maximum of the mask over the tile's pixels inside
// the frame.  The caller has checked: width, height >= 1, 1 <= lo <= hi <= 64
void emphasis_from_mask(const uint8_t* mask, int width, int height, size_t row_stride, int lo, int hi, uint8_t* emphasis);

// ---- a group of frames (include/mpcodec.h, "group"; DESIGN.md 4, "Encoder: a group of frames") ----
// `frames` frames of one geometry, `tiles` tiles each, everything frame-major: tile f * tiles + t, weights[f * 3K + ch * K + i] frame f's
// own, emphasis null or frames * tiles bytes.  One multiplier across all tiles of all frames: the squared error of a cut is additive over
// tiles whichever frame a tile belongs to, so this is the equal-slope allocation across frames as well as within them.
constexpr int kGroupMaxFrames = 64;
// For every frame f exactly budget_allocate_emphasis of frame f's profile, counts, weights and map slice at j; totals[3 * f + k] are
// that frame's.  A loop of its own over all tiles of the group -- not `frames` calls of budget_allocate_emphasis, so that the two check
// each other.  The caller has checked: 1 <= frames <= 64, and what budget_allocate's has
void budget_allocate_group(const uint32_t* profile, const uint16_t* counts, const uint8_t* emphasis, int frames, long long tiles, int K,
                           const uint32_t* weights, int j, uint8_t* depth, uint16_t* out_counts, uint64_t* totals);
// totals[3 * j + k] = the sum over f of budget_sweep_emphasis's of frame f.  A loop of its own, as budget_sweep is
void budget_sweep_group(const uint32_t* profile, const uint16_t* counts, const uint8_t* emphasis, int frames, long long tiles, int K,
                        const uint32_t* weights, uint64_t totals[3 * kBudgetLambdas]);

template <class Psnr>
uint64_t sse_for_psnr(double target, uint64_t limit, Psnr psnr) {
    uint64_t lo = 0, hi = limit;                        // psnr(lo) >= target always: psnr(0) = +inf
    if (psnr(hi) >= target) return hi;
    while (hi - lo > 1) {                               // psnr(hi) < target
        const uint64_t mid = lo + (hi - lo) / 2;
        if (psnr(mid) >= target) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace mpc
