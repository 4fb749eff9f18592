// host_rate.h -- product: the host's definitions behind a delta stream to a byte budget (include/mpcodec.h, "rate"; DESIGN.md 4,
// "Delta stream to a byte budget"): which tiles a call may send, and the allocation at one multiplier when a tile has a floor.
// Knows neither HIP nor the C ABI and builds on its own with host_budget.
#pragma once

#include <cstddef>
#include <cstdint>

namespace mpc {

// full(t) = max over ch of min(counts[t * 3 + ch], K); tile t is OWED iff sent[t] < full(t).  The candidates are the changed tiles
// (changed[n_changed], ascending, distinct, inside [0, tiles): the caller has checked) and the owed ones, ascending:
// candidates[0 .. return value).  Per TILE: must[t] = 1 iff t is changed; floor[t] = 0 for a changed tile, else sent[t].
// candidates, floor, must: each may be null; room for `tiles` entries
long long owed_tiles(const uint8_t* sent, const uint16_t* counts, long long tiles, int K, const int32_t* changed, long long n_changed,
                     int32_t* candidates, uint8_t* floor, uint8_t* must);

// budget_allocate (host_budget.h) with a floor: per candidate i its profile[i * (K + 1) + n], counts[i * 3 + ch], floor[i] (a floor
// above K is used as K) and must[i].  Allowed depths: 0 ... K when must[i], else floor[i] ... K.  R'(i, n) = R(i, n), except
// R'(i, floor[i]) = 0 when must[i] == 0: a tile that stays as the receiver holds it costs nothing.  J = P * 65536 + L[j] * R' in u64;
// depth[i] = the smallest allowed n that minimises J; send[i] = must[i] || depth[i] > floor[i]; out_counts = min(count, depth[i]);
// totals[0] = sum P[i][depth], [1] = sum R'(i, depth), [2] = the records kept in the tiles sent, [3] = the tiles sent.
// floor, must: null = all 0, all 1 (then totals[0 .. 2], depth and out_counts are budget_allocate's).  depth, out_counts, send: each
// may be null.  The caller has checked: 1 <= K <= 32, 0 <= j < 256, n >= 0
void budget_allocate_floor(const uint32_t* profile, const uint16_t* counts, const uint8_t* floor, const uint8_t* must, long long n, int K,
                           const uint32_t* weights, int j, uint8_t* depth, uint16_t* out_counts, uint8_t* send, uint64_t totals[4]);

// budget_allocate_floor with an emphasis map (host_budget.h, "emphasis"): J = P * e * 4096 + L[j] * R', candidate i taking
// e[list[i]], list == null the identity; a list entry outside [0, tiles) takes the neutral value.  totals[0] stays unweighted.
// emphasis[tiles], null = neutral: then budget_allocate_floor itself, bit for bit, whatever the list
void budget_allocate_floor_emphasis(const uint32_t* profile, const uint16_t* counts, const uint8_t* floor, const uint8_t* must,
                                    const uint8_t* emphasis, const int32_t* list, long long tiles, long long n, int K, const uint32_t* weights,
                                    int j, uint8_t* depth, uint16_t* out_counts, uint8_t* send, uint64_t totals[4]);

}  // namespace mpc
