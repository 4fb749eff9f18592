"""The harness of the stream-contract tests (tests/test_gpu_stream_order.py, tests/test_gpu_stream_capture.py).

`behind_delay` drives one entry point on a caller's stream S (a torch stream: non-blocking, the null stream does not wait for it) so
that an ordering mistake shows in what a consumer ON THAT STREAM sees.  The device buffers of the inputs hold B, a valid input whose
result differs from A's; the outputs hold poison.  Then, on S and with no host synchronisation in between:
    1. a finite delay (torch.cuda._sleep);  2. device-to-device copies that put A into the inputs (and poison into the outputs once
    more);  3. the entry point;
    4. a copy of every output into a second buffer (the consumer);  5. the inputs overwritten with B again (write after read).
A helper kernel or copy that the library puts on another stream runs while the delay still holds the copies of step 2 back: it reads
B or writes into poison.  A fork without a join lets step 4 or 5 overtake the work.  Every buffer travels as bytes.

The delay is never a kernel that waits for the host: an entry point may legitimately wait for the stream, and would then never return."""
import time

import numpy as np

POISON = 0x2A                                   # pure outputs before the call
UNSEEN = 0xEE                                   # the consumer's buffers before the copy
DELAY_FLOOR_MS, DELAY_CAP_MS = 20.0, 200.0


def cycles_per_ms(torch):
    """torch.cuda._sleep's unit, measured once with events on the current stream"""
    torch.cuda._sleep(1_000_000)                # the first launch pays for loading the kernel
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    probe = 20_000_000
    a.record()
    torch.cuda._sleep(probe)
    b.record()
    b.synchronize()
    return probe / a.elapsed_time(b)


def delay_ms_for(host_ms):
    """ten times what the host took to enqueue the same sequence in the warm-up, within [20, 200] ms"""
    return min(max(10.0 * host_ms, DELAY_FLOOR_MS), DELAY_CAP_MS)


def _bytes(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


class Buffers:
    """what a case's `call` gets: ptr(name) of every device buffer, and probe(), which it calls right behind the entry point"""

    def __init__(self, tensors, stream, probe):
        self._t, self.stream, self.probe = tensors, stream, probe

    def ptr(self, name):
        return self._t[name].data_ptr()


def behind_delay(torch, S, call, inputs, outputs, cycles, lib_stream=None):
    """inputs: {name: (A, B)} numpy arrays of one size; outputs: {name: like} -- a name that is also an input is an in/out buffer, any
    other is pre-filled with POISON (like: an array of its dtype and shape).  call(buffers): enqueues the entry point on buffers.stream
    and calls buffers.probe() right behind it; what it returns (host data of calls that have some) is handed back.
    lib_stream: the stream the library is told (default: S itself; the control passes 0).
    -> (seen {name: array like `like`}, returned, info): info["running"]: S.query() was False in probe(), i.e. the delay was still
    running when the entry point returned; info["host_ms"]: host time of steps 1 to 5."""
    dev, src_a, src_b, seen = {}, {}, {}, {}
    for name, (a, b) in inputs.items():
        assert _bytes(a).size == _bytes(b).size, name
        src_a[name], src_b[name] = torch.from_numpy(_bytes(a).copy()).cuda(), torch.from_numpy(_bytes(b).copy()).cuda()
        dev[name] = src_b[name].clone()
    for name, like in outputs.items():
        if name not in dev:
            dev[name] = torch.full((_bytes(like).size,), POISON, dtype=torch.uint8, device="cuda")
        seen[name] = torch.full((_bytes(like).size,), UNSEEN, dtype=torch.uint8, device="cuda")
    info = {"running": None}

    def probe():
        info["running"] = not S.query()

    torch.cuda.synchronize()                                        # the set-up ran on the null stream, which S does not wait for
    t0 = time.perf_counter()
    with torch.cuda.stream(S):
        torch.cuda._sleep(int(cycles))
        for name in inputs:
            dev[name].copy_(src_a[name], non_blocking=True)
        for name in outputs:                                        # poison once more, on S: a helper that ran early on another stream (a
            if name not in inputs:                                  # memset of the records, say) is undone and shows
                dev[name].fill_(POISON)
        returned = call(Buffers(dev, S.cuda_stream if lib_stream is None else lib_stream, probe))
        for name in outputs:
            seen[name].copy_(dev[name], non_blocking=True)
        for name in inputs:
            dev[name].copy_(src_b[name], non_blocking=True)
    info["host_ms"] = (time.perf_counter() - t0) * 1e3
    S.synchronize()
    got = {name: seen[name].cpu().numpy().view(np.asarray(like).dtype).reshape(np.asarray(like).shape) for name, like in outputs.items()}
    torch.cuda.synchronize()                                        # the control's work was on the null stream
    return got, returned, info


# ---- records as the device holds them, and the numpy models of the kernels that have none in a *_cases.py ----
def device_records(oracle_out, K):
    """oracle.encode_tiles' five arrays -> (counts u16 [T, 3], words u32 [T, 3, K], energy, swept): records 0 .. count as the oracle wrote
    them, every entry beyond zero (include/mpcodec.h: d_choices)"""
    oc, od, ok, oe, os_ = oracle_out
    words = od.astype(np.uint32) | (ok.astype(np.uint32) << 16)
    live = np.arange(K)[None, None, :] <= np.minimum(oc.astype(np.int64), K - 1)[:, :, None]
    return oc.astype(np.uint16), np.where(live, words, 0).astype(np.uint32), np.ascontiguousarray(oe, np.float64), os_.astype(np.uint32)


def histogram(counts, words, K, bins=8192):
    h = np.zeros((1 + 6 * K, bins), np.uint32)
    h[0] = np.bincount(counts.reshape(-1), minlength=bins)
    for ch in range(3):
        for i in range(K):
            m = counts[:, ch] > i
            h[1 + 2 * K * ch + 2 * i] = np.bincount(words[m, ch, i] & 0xFFFF, minlength=bins)
            h[2 + 2 * K * ch + 2 * i] = np.bincount(words[m, ch, i] >> 16, minlength=bins)
    return h


def crop(counts, words, tiles_y, grid, steps, K):
    """mp_device.h: launch_crop_records.  grid = (tx0, tx1, ty0, ty1)"""
    tx0, tx1, ty0, ty1 = grid
    source = (np.arange(tx0, tx1)[:, None] * tiles_y + np.arange(ty0, ty1)[None, :]).reshape(-1)
    c = np.minimum(counts[source].astype(np.int64), steps)
    return c.astype(np.uint16), np.where(np.arange(K)[None, None, :] < c[:, :, None], words[source], 0).astype(np.uint32)


def paste(counts, words, src_ty, grid, dst_counts, dst_words, dst_ty, at, K):
    """mp_device.h: launch_paste_records without an owner map -> copies of the destination with the grid pasted at tile `at`"""
    tx0, tx1, ty0, ty1 = grid
    dst_counts, dst_words = np.array(dst_counts), np.array(dst_words)
    src = (np.arange(tx0, tx1)[:, None] * src_ty + np.arange(ty0, ty1)[None, :]).reshape(-1)
    dst = ((np.arange(tx0, tx1) - tx0 + at[0])[:, None] * dst_ty + (np.arange(ty0, ty1) - ty0 + at[1])[None, :]).reshape(-1)
    c = np.minimum(counts[src].astype(np.int64), K)
    dst_counts[dst] = c.astype(np.uint16)
    dst_words[dst] = np.where(np.arange(K)[None, None, :] < c[:, :, None], words[src], 0).astype(np.uint32)
    return dst_counts, dst_words


def interleave(part_counts, part_words, tiles_x, tiles_y, a, b, frame_counts, frame_words):
    """stripe order t = tx * (b - a) + (ty - a) -> whole-frame order t = tx * tiles_y + ty, the other rows as they were"""
    fc, fw = np.array(frame_counts).reshape(tiles_x, tiles_y, 3), np.array(frame_words).reshape(tiles_x, tiles_y, 3, -1)
    fc[:, a:b] = part_counts.reshape(tiles_x, b - a, 3)
    fw[:, a:b] = part_words.reshape(tiles_x, b - a, 3, -1)
    return fc.reshape(-1, 3), fw.reshape(tiles_x * tiles_y, 3, -1)


def unpack(packed, tiles, rows_per_column, frame):
    """delta_cases.pack's inverse: listed tile j of the packed frame [8R, 8C, 3] to tile tiles[j] of a copy of `frame`, inside the image"""
    out = np.array(frame)
    h, w = out.shape[:2]
    ty = -(-h // 8)
    R = min(len(tiles), rows_per_column)
    for j, t in enumerate(tiles):
        cx, cy = divmod(int(t), ty)
        y1, x1 = min(cy * 8 + 8, h), min(cx * 8 + 8, w)
        out[cy * 8:y1, cx * 8:x1] = packed[(j % R) * 8:(j % R) * 8 + y1 - cy * 8, (j // R) * 8:(j // R) * 8 + x1 - cx * 8]
    return out


def tile_sums(a, b):
    """per tile t = tx * tiles_y + ty the sum of squared differences of two [H, W, 3] frames"""
    H, W = a.shape[:2]
    d = ((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum(axis=2)
    full = np.zeros((-(-H // 8) * 8, -(-W // 8) * 8), np.int64)
    full[:H, :W] = d
    return full.reshape(full.shape[0] // 8, 8, full.shape[1] // 8, 8).sum(axis=(1, 3)).T.reshape(-1)
