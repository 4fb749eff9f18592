"""The hand-made frames of tests/record_cases.py, checked on the CPU: the containers hold exactly the records written down, the numpy
restatement of the reference's tile decode equals the oracle on them, and every mistake the restatement can be switched to changes
pixels.  test_gpu_record_decode.py relies on all of it: a frame that lost a property would still pass there and test nothing.
Every expected pixel is the oracle's; the restatement only shows that the frames discriminate."""
import numpy as np
import pytest

import record_cases as rc
import view_cases

NAMES = tuple(rc.FRAMES)
CLAMPED_SHARE_MAX = 0.25


@pytest.fixture(scope="module")
def decoded(oracle):
    """{name: the oracle's decode of the frame's container}, computed once"""
    return {name: oracle.decode_image(rc.frame(name).container) for name in NAMES}


@pytest.fixture(scope="module")
def restated():
    cache = {}

    def get(name, mutant=None):
        if (name, mutant) not in cache:
            cache[name, mutant] = rc.decode(rc.frame(name), mutant)
        return cache[name, mutant]
    return get


def _classes_present(f):
    """what the lists of a frame show of the classes, per channel"""
    seen = [set() for _ in range(3)]
    for per_channel in f.records:
        for ch, lst in enumerate(per_channel):
            choices, qs = [c for c, _ in lst], [q for _, q in lst]
            steps = [int(s) for s in f.quant[ch][:len(lst)]]
            if not lst:
                seen[ch].add("empty")
                continue
            if len(lst) == 1 and choices == [0]:
                seen[ch].add("flat")
            if len(lst) == 2 and choices == [0, 0] and steps == [8, 1] and qs[1] % 8 == 4:
                seen[ch].add("half")
            for i, c in enumerate(choices):
                if c >= rc.NB and rc.outside(lst[:i + 1]) and not rc.outside(lst):
                    seen[ch].add("forward")
                if 0 <= c < rc.NB and qs[i] == 0 and any(x >= rc.NB for x in choices[i + 1:]):
                    seen[ch].add("zero_unlock")
            bases = [c for c in choices if c < rc.NB]
            if len(bases) != len(set(bases)):
                seen[ch].add("repeat")
            if rc.NB - 1 in choices or rc.NB in choices or rc.dictionary_size(choices) - 1 in choices:
                seen[ch].add("edge")
            if any(q in (-32768, 32767) and s != 0 for q, s in zip(qs, steps)) or any(s == 65535 and q for q, s in zip(qs, steps)):
                seen[ch].add("extreme")
            if any(steps[i:i + 2] == [60000, 59999] and qs[i:i + 2] == [20, -20] and choices[i] == choices[i + 1] for i in range(len(lst) - 1)):
                seen[ch].add("cancel")
    return seen


@pytest.mark.parametrize("name", NAMES)
def test_every_class_is_there(name):
    f = rc.frame(name)
    W, H, K, is_closed = rc.FRAMES[name]
    assert (f.W, f.H, f.K) == (W, H, K) and len(f.records) == f.tiles_x * f.tiles_y
    seen = _classes_present(f)
    everywhere = {"flat", "forward", "zero_unlock", "repeat", "edge", "extreme", "empty"} - ({"forward"} if is_closed else set())
    # 15 tiles go round the nine classes less than twice, and one Extreme list clamps most of a tile, 1/15 of the frame: all the
    # other classes in luma, every class somewhere, and in chroma what the cycle and the tiles set aside leave.  The two wide frames
    # hold every class in every channel (below)
    assert (everywhere | {"half", "cancel"}) - {"extreme"} <= seen[0], (name, seen[0])
    assert everywhere <= seen[0] | seen[1] | seen[2], (name, everywhere - (seen[0] | seen[1] | seen[2]))
    assert everywhere - {"extreme"} <= seen[1] | seen[2], (name, everywhere - (seen[1] | seen[2]))
    symbols = {int(w) >> 16 for w in f.choices.reshape(-1)}
    assert 0xFFFF in symbols and (0xFFFE in symbols or K < 7)      # q = -32768 and 32767
    assert all(not rc.outside(lst) for per_channel in f.records for lst in per_channel)
    assert all(rc.closed(lst) for per_channel in f.records for lst in per_channel) == is_closed
    # count 0 on one, two and -- but for odd_k, where one black tile is 1/15 of the frame -- all three channels
    assert {1, 2, 3} - ({3} if name == "odd_k" else set()) <= {sum(1 for lst in per_channel if not lst) for per_channel in f.records}
    assert rc.dc_symbols_round_trip(f)
    if K == 32:                                                 # a full list: 31 distinct base choices, then the last row of the 31st block
        full = [lst for per_channel in f.records for lst in per_channel if len(lst) == 32]
        assert any(len({c for c, _ in lst[:31]}) == 31 and max(c for c, _ in lst[:31]) < rc.NB and
                   lst[31][0] == rc.dictionary_size([c for c, _ in lst]) - 1 for lst in full)
        # every class on both sides of tile 1024
        for side in (slice(0, 1024), slice(1024, None)):
            part = rc.Frame("part", 8, 8 * len(f.records[side]), K, f.records[side])
            got = _classes_present(part)
            assert all(everywhere <= got[ch] for ch in range(3)) and {"half", "cancel"} <= got[0], side
    assert rc.tables(K).shape == (3, K) and np.array_equal(f.quant, rc.tables(K))
    assert {65535, 0, 60000, 59999} <= set(f.quant.reshape(-1).tolist())


@pytest.mark.parametrize("name", NAMES)
def test_the_container_holds_exactly_these_records(oracle, name):
    f = rc.frame(name)
    st = oracle.read_compressed(f.container)
    lengths, codes = f.streams()
    assert (st["W"], st["H"], st["K"], st["bs"]) == (f.W, f.H, f.K, 8)
    assert np.array_equal(st["quant"], f.quant)
    assert np.array_equal(st["lengths"], lengths)
    for i in range(6 * f.K):
        assert np.array_equal(st["codes"][i], codes[i]), (name, i)      # the step-0 coefficients un-differenced among them
    mine = oracle.write_compressed(dict(W=f.W, H=f.H, K=f.K, bs=8, quant=f.quant, lengths=lengths, codes=codes))
    assert mine == f.container


@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_is_the_oracle(decoded, restated, name):
    assert np.array_equal(restated(name), decoded[name])


@pytest.mark.parametrize("name", NAMES)
def test_every_mutant_changes_pixels(decoded, restated, name):
    f = rc.frame(name)
    tiles = len(f.records)
    sides = [range(tiles)] if tiles <= 1024 else [range(0, 1024), range(1024, tiles)]
    for mutant in rc.MUTANTS:
        changed = (restated(name, mutant) != decoded[name]).any(axis=-1)
        if mutant == "earlier_only" and rc.FRAMES[name][3]:
            # a frame without forward references: the dictionary of the earlier choices names the same rows, which is what makes
            # every prefix of it decodable
            assert not changed.any()
            continue
        for side in sides:
            assert changed[f.tile_mask(side)].any(), (name, mutant, side)
    # pixels that only U records, and only V records, account for: the other two lists are empty or the constant alone, which these
    # three mutants leave as it is; behind tile 1024 of the wide frames, where the frame can afford it, they are empty
    for mutant in ("luma_detail", "earlier_only", "no_repeat"):
        if mutant == "earlier_only" and rc.FRAMES[name][3]:
            continue
        changed = (restated(name, mutant) != decoded[name]).any(axis=-1)
        for ch in (1, 2):
            alone = [t for t in range(tiles) if not rc.plain(f.records[t][ch]) and rc.plain(f.records[t][0]) and rc.plain(f.records[t][3 - ch])]
            assert alone and changed[f.tile_mask(alone)].any(), (name, mutant, ch)
            if tiles > 1024:
                only = [t for t in alone if not f.counts[t, 0] and not f.counts[t, 3 - ch]]
                assert only and changed[f.tile_mask(only)].any(), (name, mutant, ch)


@pytest.mark.parametrize("name", NAMES)
def test_the_flavours_differ(oracle, decoded, name):
    assert (oracle.decode_image_fast(rc.frame(name).container) != decoded[name]).any()


@pytest.mark.parametrize("name", NAMES)
def test_saturation_cannot_hide_a_failure(decoded, name):
    share = float(np.isin(decoded[name], (0, 255)).mean())
    assert share <= CLAMPED_SHARE_MAX, f"{name}: {share:.4f} of the colour samples are 0 or 255"


@pytest.mark.parametrize("kind,ch,last", rc.bad_cases())
def test_bad_frames_have_one_record_outside(oracle, decoded, kind, ch, last):
    b = rc.bad("small", kind, ch, last)
    good = rc.frame("small")
    t, c, step = b.bad_at
    assert (c == ch or last) and (len(b.records[t][c]) == b.K) == last
    differing = [(tt, cc) for tt in range(len(good.records)) for cc in range(3) if good.records[tt][cc] != b.records[tt][cc]]
    assert differing == [(t, c)]
    assert sum(x != y for x, y in zip(good.records[t][c], b.records[t][c])) == 1 and len(good.records[t][c]) == len(b.records[t][c])
    for tt, per_channel in enumerate(b.records):
        for cc, lst in enumerate(per_channel):
            assert rc.outside(lst) == ([step] if (tt, cc) == (t, c) else []), (tt, cc)
    choice = b.records[t][c][step][0]
    if kind == "beyond":
        assert choice == rc.dictionary_size([x for x, _ in b.records[t][c]])
        twin = rc.bad("small", kind, ch, last, lower=1)
        assert twin.bad_at == b.bad_at and twin.records[t][c][step][0] == choice - 1
        assert all(not rc.outside(lst) for per_channel in twin.records for lst in per_channel)
        assert np.array_equal(oracle.decode_image(twin.container), rc.decode(twin))
    elif kind == "negative":
        assert choice < 0 and step >= 1
    else:
        assert (step, choice) == (0, rc.NB) and all(x >= rc.NB for x, _ in b.records[t][c])
    assert rc.dc_symbols_round_trip(b)
    # the container carries the record as written; the oracle skips it, and nothing outside that tile depends on it
    lengths, codes = b.streams()
    st = oracle.read_compressed(b.container)
    assert np.array_equal(st["lengths"], lengths) and all(np.array_equal(x, y) for x, y in zip(st["codes"], codes))
    other = ~b.tile_mask([t])
    assert np.array_equal(oracle.decode_image(b.container)[other], decoded["small"][other])


def test_every_prefix_of_the_closed_frame_decodes(oracle):
    f = rc.frame("wide_closed")
    for steps in (1, 2, 3, 31):
        cut = view_cases.truncated(f.container, steps)
        st = oracle.read_compressed(cut)
        assert np.array_equal(st["lengths"], np.minimum(f.counts.reshape(-1), steps))
        prefix = rc.Frame("prefix", f.W, f.H, f.K, [[lst[:steps] for lst in per_channel] for per_channel in f.records])
        assert all(not rc.outside(lst) for per_channel in prefix.records for lst in per_channel)
        assert prefix.container == cut
        assert np.array_equal(oracle.decode_image(cut), rc.decode(prefix))
