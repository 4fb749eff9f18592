"""A group of frames to one budget or one quality (include/mpcodec.h, "group") as a numpy model: the group allocation -- for every
frame budget_cases.allocate of that frame with its own weights (emphasis_cases.allocate where there is a map), frame by frame -- and
the group sweep, those totals summed over the frames; the cases the host functions and the two group kernels are held to; and the
mistakes every case set must tell apart (WRONG).  Imported by test_group_cases.py (CPU) and test_gpu_target_group.py; nothing here
needs the library; budget_cases.py and emphasis_cases.py are used as they are.

A case is (name, profile uint32 [F, T, K + 1], counts uint16 [F, T, 3], emphasis uint8 [F, T], weights uint32 [F, 3, K], js): every
case is run with its map and without one."""
import numpy as np

import budget_cases as bc
import emphasis_cases as ec

LAMBDAS = bc.LAMBDAS
MAX_FRAMES = 64
CHUNK = 8                                       # frames a launch takes (mp_device.h: kGroupChunk)
KS = (1, 8, 32)
TILE_COUNTS = (1, 3, 15, 17, 25, 33)            # below a workgroup's four waves, off their multiple, either side of the sweep's 16-tile run
FRAME_COUNTS = (1, 2, 3, 5, 9)                  # 9 crosses a chunk of 8
JS = (0, 1, 40, 90, 120, 160, 200, 255)

WRONG = ("frame 0's weights for every frame", "weights of frame f + 1", "a 16-tile run continues into the next frame",
         "a 4-tile workgroup continues into the next frame", "totals summed into frame 0", "emphasis slice at offset 0 for every frame",
         "sweep without the last frame")
WRONG_ALLOCATE = WRONG[:6]                      # the last is the sweep's alone
NEEDS_MAP = ("emphasis slice at offset 0 for every frame",)


def _weights_frame(F, T, mistake):
    """[F, T]: the frame whose weights tile t of frame f is rated with"""
    own = np.repeat(np.arange(F), T).reshape(F, T)
    if mistake == "frame 0's weights for every frame":
        return np.zeros((F, T), np.int64)
    if mistake == "weights of frame f + 1":
        return (own + 1) % F
    for label, run in (("a 16-tile run continues into the next frame", 16), ("a 4-tile workgroup continues into the next frame", 4)):
        if mistake == label:                    # a run over the group's tiles, frame-major, keeps the weights of its first tile's frame
            g = np.arange(F * T)
            return ((g // run * run) // T).reshape(F, T)
    return own


def allocate_group(profile, counts, emphasis, weights, j, mistake=None):
    """-> (depth uint8 [F, T], cut counts uint16 [F, T, 3], totals [F][3] as Python ints): frame f is emphasis_cases.allocate (without a
    map budget_cases.allocate's result) of its own profile, counts, map slice and weights"""
    profile = np.asarray(profile, np.uint32)
    F, T, K = profile.shape[0], profile.shape[1], profile.shape[2] - 1
    counts = np.asarray(counts, np.uint16).reshape(F, T, 3)
    emphasis = None if emphasis is None else np.asarray(emphasis, np.uint8).reshape(F, T)
    wf = _weights_frame(F, T, mistake)
    depth, cut, totals = np.zeros((F, T), np.uint8), np.zeros((F, T, 3), np.uint16), [[0, 0, 0] for _ in range(F)]
    for f in range(F):
        e = None if emphasis is None else emphasis[0 if mistake == "emphasis slice at offset 0 for every frame" else f]
        for w in np.unique(wf[f]):
            at = np.nonzero(wf[f] == w)[0]
            d, c, t = ec.allocate(profile[f][at], counts[f][at], None if e is None else e[at], weights[w], j)
            depth[f][at], cut[f][at] = d, c
            into = totals[0 if mistake == "totals summed into frame 0" else f]
            for k in range(3):
                into[k] += t[k]
    return depth, cut, totals


def sweep_group(profile, counts, emphasis, weights, mistake=None, js=range(LAMBDAS)):
    """{j: [distortion, rate, records]}: the group allocation's totals summed over the frames"""
    F = np.asarray(profile).shape[0]
    frames = F - 1 if mistake == "sweep without the last frame" else F
    out = {}
    for j in js:
        totals = allocate_group(profile, counts, emphasis, weights, j, mistake)[2]
        out[j] = [sum(totals[f][k] for f in range(frames)) for k in range(3)]
    return out


def octave_weights(rng, F, K):
    """every frame's own, frame to frame apart by octaves (a textured frame's records cost a multiple of a flat one's), inside the clamp"""
    return np.stack([np.minimum(bc._weights(rng, K).astype(np.int64) << (f * 2 % 6), bc.W_MAX) for f in range(F)]).astype(np.uint32)


def cases():
    rng = np.random.default_rng(20241021)
    out = []
    for K in KS:
        for F in FRAME_COUNTS:
            for T in TILE_COUNTS:
                counts = rng.integers(0, K + 1, (F, T, 3)).astype(np.uint16)
                counts[rng.random((F, T)) < 0.1] = 0
                label = f"K{K} F{F} T{T}"
                if F >= 3 and T == 17:
                    counts[1] = 0                                                    # one frame with all counts 0
                    label += " frame 1 empty"
                if T == 25:
                    counts[F - 1, 3, 1], counts[0, 24, 2] = K + 1, 65535             # counts above K are used as K
                    label += " counts above K"
                P = np.stack([bc._consistent_profile(rng, np.minimum(counts[f], K), K, monotone=(F % 2 == 0)) for f in range(F)])
                E = rng.integers(1, ec.E_MAX + 1, (F, T)).astype(np.uint8)
                E.reshape(-1)[::5] = np.resize(np.array([0, 1, ec.NEUTRAL, ec.E_MAX, 255], np.uint8), E.reshape(-1)[::5].size)
                out.append((label, P, counts, E, octave_weights(rng, F, K), JS))
    return out


def told_apart(case, mistake, with_map):
    """whether the model with `mistake` gives another result than the model on this case"""
    _, P, counts, E, W, js = case
    E = E if with_map else None
    if mistake == "sweep without the last frame":
        return sweep_group(P, counts, E, W, js=js) != sweep_group(P, counts, E, W, mistake, js=js)
    for j in js:
        good, bad = allocate_group(P, counts, E, W, j), allocate_group(P, counts, E, W, j, mistake)
        if not (np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1]) and good[2] == bad[2]):
            return True
    return False
