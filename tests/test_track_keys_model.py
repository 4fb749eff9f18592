"""The grouped top-two tracking of the pursuit kernel (TopKeys::see4: four keys in nine instructions) against its definition (four
TopKeys::see), on the numpy model of tests/track_keys_cases.py.  Equality of the uint32 keys, no tolerance.

The device runs the same comparison on the kernel's own functions in tests/test_gpu_track_keys.py, against this model.

NaN and infinity bit patterns are out of scope: a tile-channel whose residual norm or pair bound is not below kHuge is diverted
(`odd`, `oddp` in mp_pursuit.hip) to the exhaustive evaluation before any key is read, so no record depends on how the tracking
orders them -- and the kernel's float median and the model's integer median differ exactly there."""
import numpy as np

import track_keys_cases as tk


def both(k1, k2, keys):
    s = tk.see4_sequential(k1, k2, keys)
    g = tk.see4_grouped(k1, k2, keys)
    assert np.array_equal(s[0], g[0]) and np.array_equal(s[1], g[1])
    assert (s[0] >= s[1]).all()
    return s


def groups_from(state_and_values, keep):
    """[n, 6] bit patterns -> state (the first two as keys with codes 0 and 1 of an earlier tile, sorted) and four keys with the
    codes of a later tile"""
    b = tk.u32(state_and_values)
    s = np.sort(np.stack([tk.make_key(b[:, 0], keep, 0), tk.make_key(b[:, 1], keep, 1)]), axis=0)
    keys = [tk.make_key(b[:, 2 + v], keep, 4 + v) for v in range(4)]
    return s[1], s[0], keys


def test_every_ordering_of_six_distinct_keys():
    perms = tk.orderings_of_six()
    assert perms.shape == (720, 6)
    for keep in (tk.KEEP_ROW, tk.KEEP_PAIR):
        k1, k2, keys = groups_from(perms, keep)
        assert len({int(x) for x in np.concatenate([k1[:1], k2[:1]] + [k[:1] for k in keys])}) == 6      # distinct under the mask
        n1, n2 = both(k1, k2, keys)
        allk = np.sort(np.stack([k1, k2] + keys), axis=0)
        assert np.array_equal(n1, allk[-1]) and np.array_equal(n2, allk[-2])      # and they are the two largest


def test_random_groups():
    rng = np.random.default_rng(12345)
    for keep in (tk.KEEP_ROW, tk.KEEP_PAIR):
        k1, k2, keys = groups_from(tk.finite_bits(rng, (10000, 6)), keep)
        both(k1, k2, keys)


def test_values_equal_before_the_code():
    rng = np.random.default_rng(777)
    for keep in (tk.KEEP_ROW, tk.KEEP_PAIR):
        b = np.repeat(tk.finite_bits(rng, (2000, 1)), 6, axis=1)
        b[1000:, 2:] ^= np.uint32(0x80000000)                        # the sign is masked away as well
        k1, k2, keys = groups_from(b, keep)
        n1, n2 = both(k1, k2, keys)
        assert ((n1 & keep) == (n2 & keep)).all() and (n1 != n2).all()


def test_all_zero_groups():
    zero = np.zeros(1, np.uint32)
    n1, n2 = both(zero, zero, [tk.make_key(0, tk.KEEP_ROW, c) for c in range(4)])
    assert (int(n1[0]), int(n2[0])) == (3, 2)                       # the codes alone
    n1, n2 = both(zero, zero, [zero] * 4)
    assert (int(n1[0]), int(n2[0])) == (0, 0)


def test_largest_finite_value():
    top = np.full(1, tk.FLT_MAX_BITS, np.uint32)
    for keep, codes in ((tk.KEEP_ROW, 127), (tk.KEEP_PAIR, 511)):
        keys = [tk.make_key(top, keep, codes - v) for v in range(4)]
        n1, n2 = both(np.zeros(1, np.uint32), np.zeros(1, np.uint32), keys)
        assert (int(n1[0]), int(n2[0])) == (tk.FLT_MAX_BITS, tk.FLT_MAX_BITS - 1)
        n1, n2 = both(n1, n2, [tk.make_key(v, keep, 0) for v in (0, 1, tk.FLT_MAX_BITS, 0x00800000)])
        assert (int(n1[0]), int(n2[0])) == (tk.FLT_MAX_BITS, tk.FLT_MAX_BITS - 1)


def test_a_wave_as_the_kernel_lays_it_out():
    """the device test's launches on the model: 36 tiles x 4 values and 16 pair values per lane"""
    for name, row_bits, pair_bits, bound, rows, pair in tk.device_cases():
        s = tk.track_rows(row_bits, tk.see4_sequential)
        g = tk.track_rows(row_bits, tk.see4_grouped)
        assert all(np.array_equal(x, y) for x, y in zip(s, g)), name
        sp = tk.track_pair(pair_bits, bound, rows, pair, tk.see4_sequential)
        gp = tk.track_pair(pair_bits, bound, rows, pair, tk.see4_grouped)
        assert all(np.array_equal(x, y) for x, y in zip(sp, gp)), name
        exp = (np.concatenate([x for x in s] + [sp[0], sp[1]]) >> 23) & 0xFF
        assert (exp != 0xFF).all(), name                             # the cases stay finite
    # the orderings case does put every ordering in front of a group of four
    bits = tk.rows_with_every_ordering()
    seen = {tuple(int(x) & 0xFFFFFF for x in np.concatenate([bits[l, 8 * j: 8 * j + 2], bits[l, 8 * j + 4: 8 * j + 8]]))
            for l in range(tk.LANES) for j in range(18)}
    assert len(seen) == 720


def test_pad_rows_of_a_pair_have_key_zero():
    p = np.full((tk.LANES, 16), np.float32(1.5).view(np.uint32), np.uint32)
    for rows, zeroed in ((62, (14, 15)), (63, (15,)), (64, ())):
        k1, k2, big = tk.track_pair(p, 0.25, rows, 0, tk.see4_sequential)
        want = np.float32(1.75).view(np.uint32) & tk.KEEP_PAIR
        last = max(i for i in range(16) if i not in zeroed)
        assert (k1[48:] == (want | np.uint32(last))).all() and (k1[:48] == (want | np.uint32(15))).all()
        assert (big == np.float32(1.5).view(np.uint32)).all()
