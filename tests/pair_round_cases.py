"""Inputs of the pair-round tests (test_pair_round_cases.py on the CPU, test_gpu_pair_rounds.py on the device), and what the
oracle's records say about them.

The pursuit kernel updates the kept approximations of a wave's pairs (a tile-channel and a detail block it has unlocked) in
rounds of 16 ITEMS; an item is pair p of a slot that goes on, other than the pair the step has just created.  A wave takes 16
consecutive vectors of a calc_mp batch, so a GROUP of 16 vectors is one wave's slots and the number of items of every step
follows from the records alone.

A vector of a group is sum_j 900 * 0.8^j * base[r_j] over m distinct base rows (none of them row 0, whose block is not a
pair): the pursuit picks them roughly in order of weight, every first pick of a base row unlocks its block, and m sets how many
pairs the vector collects and when it ends.  Every group runs in the "tiny" form of pursuit_cases.py with ONE step for the whole
group (the quantiser is an argument of the call): the pursuit goes on until the residual is rounding noise."""
import numpy as np

import pursuit_cases as pc

K = 32
NUM_BASE = 510

RAMP = list(range(16))
MIXED = [0, 1, 2, 3, 12, 1, 0, 25, 4, 0, 18, 1, 7, 0, 30, 2]
GROUPS = {                       # name -> rows per vector (a multiple of 16 vectors: whole waves)
    "ramp": RAMP,
    "deep": [20] * 16,
    "mixed": MIXED,
    "one": [1] * 16,
    # wave 0 is the ramp reversed, waves 1 .. 3 the same rotated by 5 slots each: their levels meet the round boundaries elsewhere
    "ramp_reversed_4_waves": [(15 - i + 5 * w) % 16 for w in range(4) for i in range(16)],
}


def group_vectors(base, name):
    """float64 [n, 64], f32-valued (both flavours take the same numbers)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    out = []
    for m in GROUPS[name]:
        rows = rng.choice(np.arange(1, base.shape[0]), size=m, replace=False)
        v = np.zeros(64)
        for j, r in enumerate(rows):
            v = v + 900.0 * 0.8 ** j * base[r]
        out.append(v)
    return pc.as_f32(np.array(out))


def group_quant(v):
    """one tiny step for the whole group: pursuit_cases.tiny_quant of its largest element"""
    return pc.tiny_quant(v, K)


def chosen_ids(count, delta):
    """dictionary indices of the atoms of one vector from its records (delta / zig-zag of MatchingPursuit.cpp:50-71)"""
    ids, prev = [], 0
    for s in range(int(count)):
        d = int(delta[s])
        prev = d if s == 0 else prev + ((d >> 1) ^ -(d & 1))
        ids.append(prev)
    return ids


def items_per_step(count, delta):
    """items[s] = pairs of the vector that the pair phase at the end of step s updates: the pairs created by the steps before
    s, if the vector goes on after s (s < count and s + 1 < K), else 0.  fresh_only[s]: it goes on and its only pair is the
    one step s created.  Also the final number of pairs."""
    ids = chosen_ids(count, delta)
    created_at, seen = [], set()
    for s, i in enumerate(ids):
        goes_on = s + 1 < K
        new = goes_on and 0 < i < NUM_BASE and i not in seen
        if i < NUM_BASE:
            seen.add(i)
        created_at.append(bool(new))
    items, fresh_only = [0] * K, [False] * K
    have = 0
    for s in range(K):
        goes_on = s < count and s + 1 < K
        if goes_on:
            items[s] = have
            fresh_only[s] = have == 0 and created_at[s]
            have += 1 if created_at[s] else 0
    return items, fresh_only, have


def analyse(counts, deltas):
    """a group of 16 vectors (one wave) -> what its steps ask of the pair rounds"""
    per = [items_per_step(counts[i], deltas[i]) for i in range(len(counts))]
    totals = [sum(p[0][s] for p in per) for s in range(K)]
    going = [sum(1 for i in range(len(counts)) if s < counts[i] and s + 1 < K) for s in range(K)]
    return {
        "totals": totals,
        "max_pairs": max(p[2] for p in per),
        "fresh_only": any(any(p[1]) for p in per),
        "ends_early": any(0 < going[s] < going[0] for s in range(K)),
        "counts": [int(c) for c in counts],
    }
